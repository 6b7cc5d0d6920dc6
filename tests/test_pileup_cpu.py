"""CPU tests (no GPU) of the per-base pileup (analyzer --pileup, t1k_pileup_*): the usage text, the C-ABI export, hand-worked
alignments through the sequential restatement (pileup_ref) the GPU tests compare the kernel and the analyzer against, and the
restatement's invariants on a generated table."""
import ctypes as C
import os
import subprocess

import numpy as np

import pileup_ref as ref
import util
import t1k_amd

ANALYZER = os.path.join(util.ROOT, "t1k_amd", "bin", "analyzer")
NAMES = ref.COUNTERS


def test_analyzer_usage_lists_the_pileup_flag(built):
    r = subprocess.run([ANALYZER], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0
    assert "--pileup:" in r.stderr and "prefix_allele_pileup.tsv" in r.stderr


def test_pileup_symbols_exported(built):
    L = C.CDLL(t1k_amd.lib_path())
    for name in ("t1k_pileup_begin", "t1k_pileup_add", "t1k_pileup_get", "t1k_pileup_end"):
        assert hasattr(L, name), name
    assert hasattr(t1k_amd.Context, "pileup")
    assert t1k_amd.PILEUP_ALN_DTYPE.itemsize == 40 and len(NAMES) == 14


def test_no_allele_selected_gives_the_header_alone(built, tmp_path):
    """an empty <prefix>_allele.tsv: the analyzer loads nothing and touches no GPU; the pileup is its header"""
    empty = tmp_path / "none_allele.tsv"
    empty.write_text("")
    o = str(tmp_path / "o")
    base = [ANALYZER, "-f", str(tmp_path / "ref.fa"), "-a", str(empty), "-u", str(tmp_path / "r.fq"), "-o", o]
    r = subprocess.run(base + ["--pileup"], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert open(o + "_allele_pileup.tsv").read() == ref.HEADER + "\n" and open(o + "_allele.vcf").read() == ""
    os.remove(o + "_allele_pileup.tsv")
    r = subprocess.run(base, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and not os.path.exists(o + "_allele_pileup.tsv")


def _cells(counts, off=0):
    """{(position, counter name): value} of the cells that are not zero"""
    return {(int(p) - off, NAMES[c]): int(counts[c, p]) for c, p in zip(*np.nonzero(counts))}


def _one(o1, e1, read1, allele_len=(10,), o2=None, e2=(), read2=None, from2=0, more=()):
    ptr, asg, ops = ref.assignments([[(o1[0], o1, e1, o2, e2, from2)] + list(more)])
    got = ref.restate(ptr, asg, ops, [read1], [read2 if read2 is not None else read1], list(allele_len))
    assert np.array_equal(got, ref.restate_by_loops(ptr, asg, ops, [read1], [read2 if read2 is not None else read1], list(allele_len)))
    return got


def test_insert_as_first_op_books_at_seq_start():
    got = _one(ref.overlap(0, 0, 2, 4, 5), [2, 0, 0], "GAC")
    assert _cells(got) == {(4, "ins"): 1, (4, "ins_uniq"): 1, (4, "A"): 1, (4, "A_uniq"): 1, (5, "C"): 1, (5, "C_uniq"): 1}


def test_insert_as_last_op_books_at_the_last_consumed_position():
    got = _one(ref.overlap(0, 1, 4, 2, 3), [0, 1, 2, 2], "TACGT")      # the window starts at read position 1
    assert _cells(got) == {(2, "A"): 1, (3, "C"): 1, (3, "ins"): 2, (2, "A_uniq"): 1, (3, "C_uniq"): 1, (3, "ins_uniq"): 2}   # ins counts bases, not events


def test_all_insert_window_at_the_alleles_end_is_clamped():
    got = _one(ref.overlap(0, 0, 1, 10, 9), [2, 2], "AC")             # seq_start one past the last base, nothing consumed
    assert _cells(got) == {(9, "ins"): 2, (9, "ins_uniq"): 2}
    got = _one(ref.overlap(0, 0, 2, 9, 9), [0, 2, 2], "TAC")          # inserts behind the allele's last base
    assert _cells(got) == {(9, "T"): 1, (9, "ins"): 2, (9, "T_uniq"): 1, (9, "ins_uniq"): 2}


def test_delete_run():
    got = _one(ref.overlap(0, 0, 1, 3, 7), [0, 3, 3, 3, 0], "GT")
    want = {(3, "G"): 1, (4, "del"): 1, (5, "del"): 1, (6, "del"): 1, (7, "T"): 1}
    want.update({(p, n + "_uniq"): v for (p, n), v in list(want.items())})
    assert _cells(got) == want
    depth = got[:6].sum(axis=0)
    assert depth[3:8].tolist() == [1] * 5 and depth.sum() == 5


def test_unknown_read_bytes_count_as_n():
    got = _one(ref.overlap(0, 0, 3, 0, 3), [0, 0, 1, 0], "ANnC")
    assert _cells(got) == {(0, "A"): 1, (1, "N"): 1, (2, "N"): 1, (3, "C"): 1, (0, "A_uniq"): 1, (1, "N_uniq"): 1, (2, "N_uniq"): 1, (3, "C_uniq"): 1}


def test_strand_minus_reads_the_reverse_complement():
    assert ref.revcomp("AACGNx") == b"NNCGTT"
    got = _one(ref.overlap(0, 1, 3, 5, 7, -1), [0, 0, 0], "AACGN")     # reverse complement NCGTT, window [1, 3] = CGT
    assert _cells(got) == {(5, "C"): 1, (6, "G"): 1, (7, "T"): 1, (5, "C_uniq"): 1, (6, "G_uniq"): 1, (7, "T_uniq"): 1}


def test_o1_from_r2_reads_the_second_read_only_without_a_mate_pair():
    got = _one(ref.overlap(0, 0, 1, 0, 1), [0, 0], "AA", read2="CC", from2=1)
    assert _cells(got) == {(0, "C"): 1, (1, "C"): 1, (0, "C_uniq"): 1, (1, "C_uniq"): 1}
    got = _one(ref.overlap(0, 0, 1, 0, 1), [0, 0], "AA", o2=ref.overlap(0, 0, 1, 4, 5), e2=[0, 0], read2="CC", from2=1)   # with a mate pair o1 is read 1
    assert _cells(got) == {(0, "A"): 1, (1, "A"): 1, (4, "C"): 1, (5, "C"): 1, (0, "A_uniq"): 1, (1, "A_uniq"): 1, (4, "C_uniq"): 1, (5, "C_uniq"): 1}


def test_overlapping_mates_both_book_and_two_assignments_are_not_unique():
    o1, o2 = ref.overlap(0, 0, 3, 2, 5), ref.overlap(0, 0, 3, 4, 7, -1)
    got = _one(o1, [0, 0, 0, 0], "ACGT", o2=o2, e2=[0, 0, 0, 0], read2="AAAA")          # mate 2 reads TTTT
    assert got[:6].sum(axis=0).tolist() == [0, 0, 1, 1, 2, 2, 1, 1, 0, 0]               # depth counts read-ends
    assert got[2, 4] == 1 and got[3, 4] == 1 and got[3, 5] == 2 and np.array_equal(got[:7], got[7:])   # G and T at 4, T twice at 5
    # the same fragment kept on a second allele as well: it books on both, and nowhere as unique
    two = _one(o1, [0, 0, 0, 0], "ACGT", allele_len=(10, 6), o2=o2, e2=[0, 0, 0, 0], read2="AAAA", more=[(1, ref.overlap(1, 0, 3, 1, 4), [0, 0, 0, 0])])
    assert np.array_equal(two[:7, :10], got[:7]) and two[:7, 10:].sum() == 4 and two[7:].sum() == 0


def test_restatement_invariants_on_a_generated_table():
    ptr, asg, ops, r1, r2, alen = ref.random_assignments(5)
    got = ref.restate(ptr, asg, ops, r1, r2, alen)
    assert np.array_equal(got, ref.restate_by_loops(ptr, asg, ops, r1, r2, alen))
    assert (got[7:] <= got[:7]).all() and got[7:].sum() > 0 and (got[7:] < got[:7]).any()
    mate = asg["has_mate_pair"] != 0
    assert mate.any() and (~mate).any() and (asg["o1_from_r2"][~mate] != 0).any() and (asg["o1"]["strand"] == -1).any()
    read_cols = int((asg["o1"]["read_end"] - asg["o1"]["read_start"] + 1).sum() + (asg["o2"]["read_end"] - asg["o2"]["read_start"] + 1)[mate].sum())
    seq_cols = int((asg["o1"]["seq_end"] - asg["o1"]["seq_start"] + 1).sum() + (asg["o2"]["seq_end"] - asg["o2"]["seq_start"] + 1)[mate].sum())
    assert int(got[:5].sum() + got[ref.INS].sum()) == read_cols      # base counters + ins = the read windows (weights 1)
    assert int(got[:5].sum() + got[ref.DEL].sum()) == seq_cols       # base counters + del = the allele windows
    assert got[ref.N].sum() > 0 and got[ref.INS].sum() > 0 and got[ref.DEL].sum() > 0
    # every fragment twice: every counter doubles
    n = len(ptr) - 1
    ptr2 = np.concatenate([ptr, ptr[1:] + ptr[-1]])
    twice = ref.restate(ptr2, np.concatenate([asg, asg]), ops, r1 + r1, r2 + r2, alen)
    assert len(ptr2) == 2 * n + 1 and np.array_equal(twice, 2 * got)


def test_record_weights_scale_the_counters():
    t = ref.generate(seed=2, records=400, text_bytes=4096)
    got = ref.book(t.allele_off, t.aln, t.text, t.ops)
    assert (got[7:] <= got[:7]).all()
    ones = t.aln.copy()
    ones["w_all"], ones["w_uniq"] = 1, 0
    cols = np.repeat(np.arange(len(t.aln)), t.aln["n_ops"].astype(np.int64))
    assert int(got[:7].sum()) == int(t.aln["w_all"].astype(np.int64)[cols].sum())
    assert int(ref.book(t.allele_off, ones, t.text, t.ops)[:7].sum()) == int(t.aln["n_ops"].sum())


def test_table_text_round_trip(tmp_path):
    counts = np.arange(14 * 5, dtype=np.int32).reshape(14, 5)
    text = ref.table_text(["X*01", "Y*02"], ["ACG", "TN"], [[1, 0, 1], [0, 1]], counts)
    p = tmp_path / "t.tsv"
    p.write_text(text)
    header, rows = ref.parse(str(p))
    assert header == ref.HEADER and [r[:4] for r in rows] == [("X*01", 1, 1, "A"), ("X*01", 2, None, "C"), ("X*01", 3, 2, "G"), ("Y*02", 1, None, "T"), ("Y*02", 2, 1, "N")]
    assert rows[3][4]["A"] == 3 and rows[3][4]["ins_uniq"] == 13 * 5 + 3
