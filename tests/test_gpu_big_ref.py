"""GPU tests of the assign stage on references of 32 768 .. 131 072 sequences: every branch keyed on the number of reference sequences
(DESIGN: reference-size regimes) against the oracle.  The references and reads are the designed cases of tests/big_ref_cases.py;
tests/test_big_ref_cpu.py proves without a GPU that each case hits the edge it is named for.  Each reference is written and uploaded
once per module; overlap lists are compared in order, field by field and with the similarity's bits, coverage base by base."""
import os
import subprocess

import numpy as np
import pytest

import big_ref_cases as B
import t1k_amd
import test_gpu_extract as ex
import test_gpu_pair as pr
import test_gpu_select_classes as classes
import test_gpu_select_tail as tail
import util

pytestmark = pytest.mark.gpu

SIM = 0.9
GENO = os.path.join(util.ROOT, "t1k_amd", "bin", "genotyper")


class Ref:
    """one designed reference: its FASTA, its reads, a context that holds it (made at first use) and the oracle's lists of its reads"""

    def __init__(self, A, tmp):
        self.A = A
        self.case = B.make_case(A)
        self.fa = B.write_fasta(str(tmp / ("ref%d.fa" % A)), self.case)
        self.reads = B.designed_reads(self.case)
        self.names, self.seqs, self.masks, _ = t1k_amd.load_reference_fasta(self.fa)
        assert self.seqs == self.case["seqs"]   # nothing collapsed: the families lie where the plan put them
        self.starts = np.concatenate([[0], np.cumsum([len(s) for s in self.seqs])]).astype(np.int64)
        self.ctx = None
        self.list_orc = None
        self.lists = {}

    def context(self):
        if self.ctx is None:
            self.ctx = t1k_amd.Context(ref_seq_similarity=SIM)
            self.ctx.ref_upload(self.seqs, self.masks)
        return self.ctx

    def oracle_list(self, read):
        if read not in self.lists:
            if self.list_orc is None:
                self.list_orc = util.Oracle(self.fa, similarity=SIM)
            self.lists[read] = self.list_orc.assign_read(read)
        return self.lists[read]

    def close(self):
        if self.ctx is not None:
            self.ctx.close()


@pytest.fixture(scope="module")
def refs(built, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bigref")
    made = {}

    def get(A):
        if A not in made:
            made[A] = Ref(A, tmp)
        return made[A]
    yield get
    for r in made.values():
        r.close()


def check_assign(ref, batches, label):
    """every batch through the reference's context and through a fresh oracle: every read-end's list, then the coverage the batches
    left together -- base by base on every allele an oracle list names, and nothing anywhere else"""
    ctx = ref.context()
    ctx.coverage_reset()
    orc = util.Oracle(ref.fa, similarity=SIM)
    named, n_lists, n_ovl = set(), 0, 0
    for b, batch in enumerate(batches):
        reads = [r for _, r in batch]
        ctx.reads_upload(reads)
        ctx.assign()
        counts, ovl = ctx.overlaps()
        assert int(counts.sum()) == len(ovl)
        pos = 0
        for i, (what, r) in enumerate(batch):
            o, s = orc.assign_read(r)
            g = ovl[pos:pos + counts[i]]
            pos += counts[i]
            assert tail.same_as_oracle(o, s, g), "%s batch %d read %s: oracle %d overlaps %s, gpu %d %s" % (
                label, b, what, len(o), o[:3, :7].tolist(), len(g), g[:3])
            ref.lists.setdefault(r, (o, s))
            named.update(o[:, 0].tolist())
            n_lists += 1 if len(o) else 0
            n_ovl += len(o)
    cov = ctx.coverage()
    want = np.zeros_like(cov)
    for a in named:
        want[ref.starts[a]:ref.starts[a + 1]] = orc.coverage(a, len(ref.seqs[a]))
    assert want.sum() > 0
    diff = np.nonzero(want != cov)[0]
    assert len(diff) == 0, "%s: coverage differs at %d bases, first at %d (allele %d): oracle %d gpu %d" % (
        label, len(diff), diff[0], int(np.searchsorted(ref.starts, diff[0], side="right")) - 1, want[diff[0]], cov[diff[0]])
    return n_lists, n_ovl


def batches_for(ref, kind):
    short, long_, xl = B.short_reads(ref.reads), B.long_reads(ref.reads), [(l, r) for l, r in ref.reads if l.startswith("xlong/")]
    return {"short": [short], "long": [long_ + short], "short+long": [short, long_ + short],
            "short+long+xlong": [short, long_ + short, xl + short, xl + long_]}[kind]


@pytest.mark.parametrize("A,kind", [(32768, "short"), (32769, "short"), (33300, "short+long+xlong"), (57344, "short"), (57345, "short"),
                                    (66200, "short"), (106496, "long"), (106497, "long"), (131072, "short+long")])
def test_lists_and_coverage(refs, A, kind):
    """a. every overlap list and the coverage against the oracle at -s 0.9.  A batch of short reads alone runs k_seed_groups<5>; a batch
    that holds a long320 read runs k_seed_groups<10> for all its reads, so the short reads of the high families go through the wide kernel
    there as well; xlong reads go through k_seed_long beside either.
      32 768   64 chunks, one directory mask word, 15 allele bits: the old side of every boundary
      32 769   65 chunks, two mask words, one allele in the last chunk, 16 bits
      33 300   straddle64 and small64 with both kernel widths; k_seed_long and the chain kernels' directory at chunk 64
      57 344 / 57 345     the two all-allele bitmaps last fit in the accumulators / first lie behind the list arrays (k_seed_groups<5>)
      66 200   17 allele bits: paralog, tie1200, tie2100, small128
      106 496 / 106 497   the same bitmap boundary for k_seed_groups<10>
      131 072  256 chunks, the last hot-chunk word, last_full, small255"""
    ref = refs(A)
    n_lists, n_ovl = check_assign(ref, batches_for(ref, kind), "A=%d %s" % (A, kind))
    assert n_lists >= 40 and n_ovl > 10000


def test_deferred_coverage_over_ranges(refs):
    """b. the designed reads of the 33 300 and 66 200 references through a context with deferred coverage, in several ranges that do not
    follow each other, against the oracle and against eager coverage (-s 0.8: the selection tests' contexts)"""
    for A in (33300, 66200):
        ref = refs(A)
        reads = [r for l, r in ref.reads if not l.startswith("bg/")]
        n = len(reads)
        orc = tail.oracle_lists(ref.fa, reads)
        assert max(len(o) for o, _ in orc) == (2100 if A == 66200 else 300) and sum(1 for o, _ in orc if len(o) == 0) == 2
        classes.check_ranges(ref.fa, reads, orc, [(0, n), (n // 2, n - n // 2), (3, 7), (0, n // 2)])


def test_pairing_across_bit_16(refs):
    """c. mates whose lists hold the low family and its paralog (an allele span far beyond the direct join's) and the two halves of
    tie1200, against Oracle.pair_rows on the lists the GPU made"""
    ref = refs(66200)
    mates = B.pair_mates(ref.case)
    reads = [m for _, a, b in mates for m in (a, b)]
    ctx = ref.context()
    ctx.reads_upload(reads)
    ctx.assign()
    counts, ovl = ctx.overlaps()
    e1, e2 = np.array([0, 2]), np.array([1, 3])
    frags = pr.fragment_lists(counts, ovl, e1, e2)
    for i, r in enumerate(reads):
        o, s = ref.oracle_list(r)
        assert tail.same_as_oracle(o, s, frags[i // 2][i % 2]), i
    for l in frags[0]:
        assert l["seq_idx"].min() < 1000 and l["seq_idx"].max() >= 65536 and l["seq_idx"].max() - l["seq_idx"].min() > t1k_amd.pair_direct_cap()
    for l in frags[1]:
        assert len(l) == 1200 and l["seq_idx"].min() < 65536 <= l["seq_idx"].max()
    ctx.pair(e1, e2, [0, 0])
    got = ctx.rows()
    pr.compare("pairs across bit 16", frags, [0, 0], ref.list_orc, *got)
    assert got[1].tolist() == [1, 1] and got[0].min() > 0   # (how many rows survive is the oracle's to say: compare checked it)
    ctx.pair(np.arange(4), None, [0, 0, 0, 0])
    pr.compare("single ends across bit 16", pr.fragment_lists(counts, ovl, np.arange(4), None), [0, 0, 0, 0], ref.list_orc, *ctx.rows())


@pytest.mark.parametrize("A", [33300, 131072])
def test_extraction(refs, A):
    """d. t1k_extract_batch on the large references (more than 64 chunks: the directory in more than one range pass), the designed reads
    and a repeat read, in the production shape and with the big shape forced for the whole batch (the references hold no tandem repeat
    that would fill a bucket beyond the production shape), against the extraction oracle with the context's k"""
    ref = refs(A)
    reads = [r for _, r in ref.reads if len(r) <= 320] + ["CAG" * 50, ref.seqs[A - 1][:60] + "CAG" * 20]
    k, hl = 12, 30
    orc = util.ExtractOracle(ref.fa, k=k, hit_len_required=hl)
    want = np.array([1 if orc.good(r) else 0 for r in reads], dtype=np.uint8)
    orc.close()
    assert want[-2] == 0 and 40 < int(want.sum()) < len(want)
    good, st = ex.device_flags(ref.seqs, reads, 1, k, hl, 0.8)
    assert np.array_equal(good, want), np.nonzero(good != want)[0]
    os.environ["T1K_EXTRACT_FORCE_BIG"] = "1"
    try:
        good2, st2 = ex.device_flags(ref.seqs, reads, 1, k, hl, 0.8)
    finally:
        del os.environ["T1K_EXTRACT_FORCE_BIG"]
    assert np.array_equal(good2, want) and st2["big_shape"] >= 1, st2


def test_one_sequence_beyond_the_limit_is_refused(refs, tmp_path):
    """e. 131 073 sequences: the reference uploads, assign() refuses by an argument check before any launch and names the limit, the
    context closes; the context that holds the 131 072 reference (the one of test_lists_and_coverage) still assigns correctly"""
    case = B.make_case(131073)
    fa = B.write_fasta(str(tmp_path / "ref.fa"), case)
    names, seqs, masks, _ = t1k_amd.load_reference_fasta(fa)
    assert len(seqs) == 131073
    ctx = t1k_amd.Context(ref_seq_similarity=SIM)
    try:
        ctx.ref_upload(seqs, masks)
        ctx.reads_upload([r for _, r in B.designed_reads(case)[:4]])
        with pytest.raises(t1k_amd.T1kError, match="more than 131 072 distinct sequences"):
            ctx.assign()
    finally:
        ctx.close()
    ref = refs(131072)
    wanted = ("small255/", "last_full/", "straddle64/", "none/")
    n_lists, n_ovl = check_assign(ref, [[(l, r) for l, r in ref.reads if l.startswith(wanted)]], "after the refusal")
    assert n_lists == 12 and n_ovl == 4 * (3 + 300 + 300)


def test_end_to_end_against_the_reference_binary(refs, tmp_path):
    """f. the executable on the 66 200 reference (17 allele bits) with 2 000 synthetic pairs of 2 x 60 bases, against the reference
    binary: genotype table, allele table and both aligned-read files byte for byte"""
    util.need(util.REF_BIN)
    ref = refs(66200)
    pfx = str(tmp_path / "s")
    util.synth_reads(ref.fa, pfx, pairs=2000, len=60, seed=31, fragmean=80, fragsd=8)
    args = ["-f", ref.fa, "-1", pfx + "_1.fq", "-2", pfx + "_2.fq", "-s", "0.9"]
    o_ref, o = str(tmp_path / "ref"), str(tmp_path / "gpu")
    a = subprocess.run([util.REF_BIN] + args + ["-t", "16", "-o", o_ref], stderr=subprocess.PIPE, text=True)
    assert a.returncode == 0, a.stderr[-500:]
    b = subprocess.run([GENO] + args + ["-o", o], stderr=subprocess.PIPE, text=True)
    assert b.returncode == 0, b.stderr[-800:]
    for suf in ("_genotype.tsv", "_allele.tsv", "_aligned_1.fa", "_aligned_2.fa"):
        assert open(o_ref + suf, "rb").read() == open(o + suf, "rb").read(), suf
    assert os.path.getsize(o + "_aligned_1.fa") > 50000
