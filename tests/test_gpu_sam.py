"""GPU tests of the SAM output (t1k_cigar_batch, analyzer --sam): the kernels against the restatement tests/sam_ref.py, byte
for byte, and through the independent decoder; the argument and capacity errors, none of which may touch an output array; the
analyzer's file against the restatement fed with the CPU oracle's alignments, line by line; the file against --pileup's table, the
reference FASTA and itself; every other output unchanged; the golden chain."""
import glob
import os
import subprocess

import numpy as np
import pytest

import goldens
import pileup_ref
import sam_ref as ref
import util
import t1k_amd
from t1k_amd.capi import CIGAR_FILL
from test_variants_host import oracle_dump, parse_dump

pytestmark = pytest.mark.gpu

GENO = os.path.join(util.ROOT, "t1k_amd", "bin", "genotyper")
ANALYZER = os.path.join(util.ROOT, "t1k_amd", "bin", "analyzer")
KEYS = ("cigar_ptr", "cigar", "md_ptr", "md", "nm", "ref_span")


@pytest.fixture(scope="module")
def table():
    return ref.kernel_table(seed=1, records=30000)


@pytest.fixture(scope="module")
def want(table):
    w = ref.restate(table.aln, table.ops, table.allele_off, table.text, table.clip)
    for v in w.values():
        v.setflags(write=False)
    return w


@pytest.fixture(scope="module")
def ctx(built):
    c = t1k_amd.Context()
    yield c
    c.close()


def _same(got, want):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def _strings(out, key, i):
    ptr = out[key + "_ptr"]
    return bytes(out[key][int(ptr[i]):int(ptr[i + 1])]).decode("ascii")


# ---- 1. kernels = restatement --------------------------------------------------------------------------------------------------------
def test_table_covers_the_cases(table, want):
    a, n = table.aln, table.aln["n_ops"]
    assert table.hand == 30000 and table.allele_len == [1, 63, 64, 65, 1000, 4097] and set(np.unique(a["allele"])) == set(range(6))
    assert all((n == k).sum() >= 2 for k in (1, 63, 64, 65, 127, 128, 129, 1000)) and (n[:table.hand] > 128).sum() > 1000
    assert (table.text == ord("N")).sum() > 50 and b"N" in bytes(want["md"])
    hand = {name: i + table.hand for i, name in enumerate(table.names)}
    assert _strings(want, "cigar", hand["matches 1000"]) == "1000M" and _strings(want, "md", hand["matches 1000"]) == "1000"
    assert _strings(want, "cigar", hand["3 2 alternating"]) == "1D1I" * 64 and _strings(want, "md", hand["3 2 alternating"]).startswith("0^")
    assert _strings(want, "cigar", hand["all insert"]) == "100I" and _strings(want, "md", hand["all insert"]) == "0"
    assert _strings(want, "cigar", hand["all delete"]) == "100D"
    assert _strings(want, "cigar", hand["deletion open over the seam, insert first"]) == "60M4D1I3D10M"
    assert _strings(want, "cigar", hand["clips 1000"]).startswith("1000S") and _strings(want, "cigar", hand["clips 9"]).endswith("991S")
    i = hand["largest clips"]
    assert int(want["cigar_ptr"][i + 1] - want["cigar_ptr"][i]) == 2 * 128 + 22          # the CIGAR bound, attained
    for length in (9, 10, 99, 100, 999, 1000):
        for cls, letter in ((0, "M"), (2, "I"), (3, "D")):
            assert _strings(want, "cigar", hand["run of %d x %d alone" % (length, cls)]) == "%d%s" % (length, letter)
    nb = n.astype(np.int64)
    assert (np.diff(want["cigar_ptr"].astype(np.int64)) <= 2 * nb + 22).all() and (np.diff(want["md_ptr"].astype(np.int64)) <= 3 * nb + 11).all()


def test_kernel_equals_restatement(ctx, table, want):
    got = ctx.cigar_batch(table.aln, table.ops, table.allele_off, table.text, table.clip)
    _same(got, want)
    assert got["ms"] > 0


def test_decoder_recovers_the_edit_strings(ctx, table):
    """independent of the restatement: CIGAR and MD as the device wrote them, read back by the SAM specification's rules"""
    lo = table.hand - 3000
    aln = table.aln[lo:]
    clip = np.minimum(table.clip[lo:], 1000)          # (the decoder wants a read of the CIGAR's length)
    got = ctx.cigar_batch(aln, table.ops, table.allele_off, table.text, clip)
    off = table.allele_off.astype(np.int64)
    text = bytes(table.text).decode("ascii")
    for i, r in enumerate(aln):
        e = table.ops[int(r["ops_at"]):int(r["ops_at"]) + int(r["n_ops"])]
        a, t = int(r["allele"]), int(r["seq_start"])
        read = ["x"] * int(clip[i][0])
        for o in e:                                   # a read that shows the allele's base on every match
            if o != 3:
                read.append(text[off[a] + t] if o == 0 else "x")
            t += 1 if o != 2 else 0
        read += ["x"] * int(clip[i][1])
        ops, bases = ref.decode(_strings(got, "cigar", i), _strings(got, "md", i), "".join(read))
        assert ops == e.tolist(), i
        assert bases == text[off[a] + int(r["seq_start"]):off[a] + t], i
        assert got["nm"][i] == (e != 0).sum() and got["ref_span"][i] == (e != 2).sum()


def test_no_clips_and_three_calls(ctx, table, want):
    plain = ref.restate(table.aln[-200:], table.ops, table.allele_off, table.text, None)
    _same(ctx.cigar_batch(table.aln[-200:], table.ops, table.allele_off, table.text, None), plain)
    parts = [ctx.cigar_batch(table.aln[lo:hi], table.ops, table.allele_off, table.text, table.clip[lo:hi]) for lo, hi in ((0, 7001), (7001, 19000), (19000, len(table.aln)))]
    for key in ("cigar", "md"):
        assert np.array_equal(np.concatenate([p[key] for p in parts]), want[key]), key
        sizes = np.concatenate([np.diff(p[key + "_ptr"].astype(np.int64)) for p in parts])
        assert np.array_equal(sizes, np.diff(want[key + "_ptr"].astype(np.int64)))
    for key in ("nm", "ref_span"):
        assert np.array_equal(np.concatenate([p[key] for p in parts]), want[key])


def test_empty_batch(ctx, table):
    rc, out = ctx.cigar_batch(table.aln[:0], table.ops, table.allele_off, table.text, raw=True)
    assert rc == 0 and out["cigar_ptr"].tolist() == [0] and out["md_ptr"].tolist() == [0]
    assert (out["cigar"] == CIGAR_FILL).all() and (out["md"] == CIGAR_FILL).all()


# ---- 2. errors leave the outputs as they were ---------------------------------------------------------------------------------------
def test_errors_touch_nothing(built):
    c = t1k_amd.Context()
    try:
        off = pileup_ref.offsets([8, 5])
        text = b"ACGTACGTNCGTA"
        ops = np.array([0, 0, 1, 0, 0, 4, 0, 0], np.int8)

        def rec(allele=0, seq_start=0, ops_at=0, n_ops=5, read_at=0):
            return np.array([(allele, seq_start, read_at, ops_at, n_ops, 0, 0, 0)], t1k_amd.PILEUP_ALN_DTYPE)
        good = np.concatenate([rec(), rec(allele=1, read_at=1 << 40)])          # (read_at is not looked at)
        out = c.cigar_batch(good, ops, off, text)
        _same(out, ref.restate(good, ops, off, text))
        assert bytes(out["cigar"]) == b"5M5M" and bytes(out["md"]) == b"2G22G2"

        def refused(bad, code, word=None, **kw):
            n = len(good) + len(bad)
            rc, o = c.cigar_batch(np.concatenate([good, bad]), ops, off, text, raw=True, **kw)
            assert rc == code, (rc, c.last_error())
            for k in KEYS:
                assert (o[k].view(np.uint8) == CIGAR_FILL).all() and len(o[k]) >= (n if k in ("nm", "ref_span") else 1), k
            if word:
                assert word in c.last_error(), c.last_error()
        ARG, CAP = -1, -3
        refused(rec(ops_at=3, n_ops=5), ARG)                   # op value 4
        refused(rec(allele=1, seq_start=1, n_ops=5), ARG)      # a walk one base past the allele
        refused(rec(seq_start=4, n_ops=5), ARG)                # ... of the first allele, whose bases continue into the second's
        refused(rec(allele=2), ARG)                            # an allele id equal to nAlleles
        refused(rec(ops_at=4, n_ops=5), ARG)                   # an edit string that leaves `ops`
        refused(rec(n_ops=0), ARG)                             # an empty edit string
        refused(rec(seq_start=9, n_ops=1), ARG)                # a start behind the allele
        refused(rec(), CAP, "cigar arena", cigar_cap=5)        # 6 bytes needed
        refused(rec(), CAP, "6 bytes", cigar_cap=5)
        refused(rec(), CAP, "md arena", md_cap=8)              # 9 bytes needed
        refused(rec(), CAP, "9 bytes", md_cap=8)
        for bad_off in (np.array([1, 8, 13], np.uint64), np.array([0, 8, 5], np.uint64)):
            rc, o = c.cigar_batch(good, ops, bad_off, text, raw=True)
            assert rc == ARG and all((o[k].view(np.uint8) == CIGAR_FILL).all() for k in KEYS)
        rc, o = c.cigar_batch(np.concatenate([good, rec()]), ops, off, text, raw=True, cigar_cap=6, md_cap=9)      # exactly enough
        assert rc == 0 and bytes(o["cigar"]) == b"5M5M5M" and bytes(o["md"]) == b"2G22G22G2"
        _same(c.cigar_batch(good, ops, off, text), out)        # and the context still takes sound calls
    finally:
        c.close()


# ---- the analyzer --------------------------------------------------------------------------------------------------------------------
def _run(cmd, env=None):
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def _genotype(tmp, ref_fa, pfx, single=False):
    g = os.path.join(tmp, "g")
    reads = ["-u", pfx + "_1.fq"] if single else ["-1", pfx + "_1.fq", "-2", pfx + "_2.fq"]
    _run([GENO, "-f", ref_fa] + reads + ["--barcode", pfx + "_bc.fa", "-o", g])
    return g, (["-u", g + "_aligned.fa"] if single else ["-1", g + "_aligned_1.fa", "-2", g + "_aligned_2.fa"])


def _analyze(ref_fa, g, aligned, out, extra=(), env=None, threads="4", barcode=True):
    bc = ["--barcode", g + "_aligned_bc.fa"] if barcode else []
    return _run([ANALYZER, "-f", ref_fa, "-a", g + "_allele.tsv"] + aligned + bc + ["-o", out, "-t", threads] + list(extra), env)


def _read(path):
    return open(path, "rb").read()


INDEL, NRATE = 0.002, 0.004


@pytest.mark.parametrize("single", [False, True], ids=["paired", "single"])
def test_analyzer_file(built, tmp_path, single):
    """3. the file = the restatement on the CPU oracle's alignments, whatever the pieces, the host path and the threads; 4. the file
    against --pileup's table, the reference FASTA and itself"""
    tmp = str(tmp_path)
    kw = dict(indel=INDEL, nrate=NRATE)
    ref_fa, pfx = util.several_snps_sample(tmp, 29, genes=3, pairs=2500, **kw) if single else util.several_snps_sample(tmp, 3, **kw)
    g, aligned = _genotype(tmp, ref_fa, pfx, single)
    a = os.path.join(tmp, "a")
    r = _analyze(ref_fa, g, aligned, a, ["--pileup", "--sam"], env={"T1K_DEBUG_PHASES": "1"}, barcode=False)   # (--barcode is not needed)
    assert [l for l in r.stderr.split("\n") if l.startswith("sam: ") and "alignments encoded" in l and "kernels" in l], r.stderr[-2000:]
    sel, out, names, _ = oracle_dump(tmp, ref_fa, g, aligned)
    recs1 = t1k_amd.read_fastx(aligned[1])
    ids, r1 = [x[0] for x in recs1], [x[2] for x in recs1]
    r2 = None if single else [s for _, _, s in t1k_amd.read_fastx(aligned[3])]
    ptr, asg, ops = parse_dump(out + "_fragdump.tsv", len(r1))
    ref_names, seqs, _, _ = t1k_amd.load_reference_fasta(sel)
    assert ref_names == names
    # what the sample has to hold for this test to mean something
    strings = [ops[int(x["ops1"]):int(x["ops1"]) + int(x["n_ops1"])] for x in asg] + [ops[int(x["ops2"]):int(x["ops2"]) + int(x["n_ops2"])] for x in asg if x["has_mate_pair"]]
    with_ins, with_del = sum(1 for e in strings if (e == 2).any()), sum(1 for e in strings if (e == 3).any())
    print("alignments %d, with an insert %d, with a deletion %d, fragments with several assignments %d" % (len(strings), with_ins, with_del, int((np.diff(ptr.astype(np.int64)) > 1).sum())))
    assert with_ins >= 20 and with_del >= 20 and (np.diff(ptr.astype(np.int64)) > 1).any()
    want = ref.header(names, seqs) + ref.sam_lines(names, seqs, ids, ptr, asg, ops, r1, r2)
    text = _read(a + "_aligned.sam")
    got = text.decode("ascii").split("\n")
    assert got[-1] == "" and len(got) - 1 == len(want)
    for i, (x, y) in enumerate(zip(got, want)):
        assert x == y, "line %d" % (i + 1)
    for tag, env, threads in (("piece", {"T1K_ANALYZER_PIECE": "600"}, "4"), ("nofast", {"T1K_ANALYZER_NO_FAST": "1"}, "4"), ("t1", {}, "1")):
        o = os.path.join(tmp, tag)
        _analyze(ref_fa, g, aligned, o, ["--sam"], env=env, threads=threads)
        assert _read(o + "_aligned.sam") == text, tag
    # ---- 4.
    head, sq, recs = ref.parse(a + "_aligned.sam")
    assert head[0] == ref.HD and head[-1] == ref.PG and sq == [(n, len(s)) for n, s in zip(names, seqs)]
    _, rows = pileup_ref.parse(a + "_allele_pileup.tsv")
    table = np.array([[r[4][c] for c in pileup_ref.COUNTERS] for r in rows], np.int32).T
    assert np.array_equal(ref.pileup_from_sam(got[:-1]), table)
    seq_of = dict(zip(names, seqs))
    by_name = {}
    for i, r in enumerate(recs):
        e, bases = ref.decode(r["cigar"], r["tags"]["MD"], r["seq"])
        there = seq_of[r["rname"]][r["pos"] - 1:r["pos"] - 1 + len(bases)]
        assert len(there) == len(bases) and all(x == y or "N" in (x, y) for x, y in zip(bases, there)), i
        assert r["tags"]["NM"] == sum(1 for o in e if o != 0)
        by_name.setdefault(r["qname"], []).append(r)
    for name, mine in by_name.items():
        k = mine[0]["tags"]["NH"]
        assert all((r["tags"]["HI"] == 1) == (r["flag"] & 0x100 == 0) and r["tags"]["NH"] == k and r["mapq"] == ref.mapq(k) for r in mine), name
        assert sorted(set(r["tags"]["HI"] for r in mine)) == list(range(1, k + 1))
        for hi in range(1, k + 1):
            pair = [r for r in mine if r["tags"]["HI"] == hi]
            if pair[0]["flag"] & 0x2:
                x, y = pair
                assert x["flag"] & 0x40 and y["flag"] & 0x80 and x["rnext"] == y["rnext"] == "=" and x["rname"] == y["rname"]
                assert x["pnext"] == y["pos"] and y["pnext"] == x["pos"] and x["tlen"] + y["tlen"] == 0 and x["tlen"] != 0
                assert bool(x["flag"] & 0x20) == bool(y["flag"] & 0x10) and bool(y["flag"] & 0x20) == bool(x["flag"] & 0x10)
            else:
                assert len(pair) == 1 and (pair[0]["rnext"], pair[0]["pnext"], pair[0]["tlen"]) == ("*", 0, 0)
                assert single or pair[0]["flag"] & 0x8


# ---- 5. nothing else changes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("het", [False, True], ids=["homo", "het"])
def test_nothing_else_changes(built, tmp_path, het):
    tmp = str(tmp_path)
    ref_fa, pfx = util.novel_snp_sample(tmp, het)
    g, aligned = _genotype(tmp, ref_fa, pfx)
    plain, flag, flag0 = (os.path.join(tmp, x) for x in ("plain", "flag", "flag0"))
    _analyze(ref_fa, g, aligned, plain)
    _analyze(ref_fa, g, aligned, flag, ["--sam"])
    _analyze(ref_fa, g, aligned, flag0, ["--varMaxGroup", "0", "--sam"])
    gold = os.path.join(util.GOLDEN, "analyzer_variants", "het" if het else "homo")
    for tail in ("_allele.vcf", "_barcode_expr.tsv"):
        assert _read(flag + tail) == _read(gold + tail) == _read(plain + tail), tail
    assert not os.path.exists(plain + "_aligned.sam")
    assert sorted(os.path.basename(p) for p in glob.glob(flag + "_*")) == ["flag_aligned.sam", "flag_allele.vcf", "flag_barcode_expr.tsv"]
    # no variant calling: the empty VCF, and the alignments all the same
    assert _read(flag0 + "_allele.vcf") == b"" and _read(flag0 + "_aligned.sam") == _read(flag + "_aligned.sam")
    assert _read(flag + "_aligned.sam").count(b"\n") > 3000


# ---- 6. the golden chain -------------------------------------------------------------------------------------------------------------
def test_golden_chain(built, tmp_path):
    tmp = str(tmp_path)
    c = goldens.Case("hla_synth_2x150", tmp)
    g = os.path.join(tmp, "g")
    _run([GENO] + c.args() + ["-o", g])
    aligned = ["-1", g + "_aligned_1.fa", "-2", g + "_aligned_2.fa"]
    flag = os.path.join(tmp, "flag")
    _analyze(c.ref, g, aligned, flag, c.flags + ["--sam"])
    assert _read(flag + "_barcode_expr.tsv").decode() == c.expected("analyzer_barcode_expr.tsv")
    assert _read(flag + "_allele.vcf").decode() == c.expected("analyzer_allele.vcf")
    head, sq, recs = ref.parse(flag + "_aligned.sam")
    selected = [l.split()[0] for l in open(g + "_allele.tsv") if l.strip()]
    seq = {name: s for name, _, s in util.read_fa(c.ref)}
    assert len(selected) >= 4 and [n for n, _ in sq] == selected and all(len(seq[n]) == ln for n, ln in sq)
    ids = set(x[0] for x in t1k_amd.read_fastx(aligned[1]))
    assert set(r["qname"] for r in recs) <= ids
    cols = sum(len(x[2]) for f in aligned[1::2] for x in t1k_amd.read_fastx(f))
    assert sum(len(r["seq"]) for r in recs if not r["flag"] & 0x100) >= 0.5 * cols      # most aligned read-ends have their primary line
    for r in recs[::7]:
        _, bases = ref.decode(r["cigar"], r["tags"]["MD"], r["seq"])
        there = seq[r["rname"]][r["pos"] - 1:r["pos"] - 1 + len(bases)]
        assert len(there) == len(bases) and all(x == y or "N" in (x, y) for x, y in zip(bases, there))
