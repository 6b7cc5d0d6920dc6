"""CPU tests (no GPU) of the indel table (analyzer --indels, t1k_indel_*): the command line, the C-ABI export, the resources
of the kernel, and the sequential restatement (indel_ref) the GPU tests compare the kernel and the analyzer against -- its two forms
against each other, the key layout, the normalisation as a property of the allele's sequence, and the cases its generated table has to cover."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import indel_ref as ref
import util
import t1k_amd
from test_kernel_resources_cpu import CSRC, hipcc_and_flags, kernel_metadata

ANALYZER = os.path.join(util.ROOT, "t1k_amd", "bin", "analyzer")
ENTRY_POINTS = ("t1k_indel_begin", "t1k_indel_add", "t1k_indel_get", "t1k_indel_stats", "t1k_indel_end")
N = ord("N")


@pytest.fixture(scope="module")
def table():
    return ref.generate(seed=1, records=6000)


@pytest.fixture(scope="module")
def want(table):
    return ref.restate(*ref.args(table))


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def test_analyzer_usage_lists_the_flags(built):
    r = subprocess.run([ANALYZER], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0
    assert "--indels:" in r.stderr and "prefix_allele_indel.tsv" in r.stderr and "--indelMinCount INT:" in r.stderr


def _no_allele(tmp_path, extra):
    empty = tmp_path / "none_allele.tsv"
    empty.write_text("")
    o = str(tmp_path / "o")
    return o, subprocess.run([ANALYZER, "-f", str(tmp_path / "ref.fa"), "-a", str(empty), "-u", str(tmp_path / "r.fq"), "-o", o] + extra, stderr=subprocess.PIPE, text=True)


@pytest.mark.parametrize("value", ["0", "-1", "2147483648", "99999999999999999999", "three", "3x", ""])
def test_min_count_outside_its_range_is_refused_before_any_work(built, tmp_path, value):
    o, r = _no_allele(tmp_path, ["--indels", "--indelMinCount", value])
    assert r.returncode != 0 and "--indelMinCount needs an integer from 1 to 2147483647." in r.stderr
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o_")]               # not even the files of a run without a selected allele


def test_no_allele_selected_gives_the_header_alone(built, tmp_path):
    for extra in ([], ["--indelMinCount", "1"], ["--indelMinCount", "2147483647"]):         # (no --barcode needed)
        o, r = _no_allele(tmp_path, ["--indels"] + extra)
        assert r.returncode == 0, r.stderr
        assert open(o + "_allele_indel.tsv").read() == ref.HEADER + "\n"
        os.remove(o + "_allele_indel.tsv")
    o, r = _no_allele(tmp_path, [])
    assert r.returncode == 0 and not os.path.exists(o + "_allele_indel.tsv")               # without the flag the file is not written


def test_min_count_without_the_flag_is_ignored_with_a_warning(built, tmp_path):
    o, r = _no_allele(tmp_path, ["--indelMinCount", "0"])                                  # (not even looked at)
    assert r.returncode == 0 and "--indelMinCount has no meaning without --indels: ignored." in r.stderr
    assert not os.path.exists(o + "_allele_indel.tsv")


# ---- the build -------------------------------------------------------------------------------------------------------------------------
def test_indel_symbols_declared_exported_and_bound(built):
    header = open(os.path.join(util.ROOT, "include", "t1k_gpu.h")).read()
    L = C.CDLL(t1k_amd.lib_path())
    for name in ENTRY_POINTS:
        assert re.search(r"^int %s\(t1k_ctx \*ctx" % name, header, flags=re.M), name
        assert hasattr(L, name), name
    assert all(hasattr(t1k_amd.Context, n) for n in ("indel", "indel_begin", "indel_add", "indel_get", "indel_stats", "indel_end"))


def test_indel_kernels_use_no_scratch(tmp_path):
    """both instantiations of k_indel, compiled for gfx950 with the Makefile's flags: no scratch memory, no spilled register, no LDS"""
    hipcc, flags = hipcc_and_flags()
    if shutil.which(hipcc) is None:
        pytest.skip("no hipcc")
    out = str(tmp_path / "t1k_indel.s")
    r = subprocess.run([hipcc] + flags + ["--offload-device-only", "-S", "-o", out, "t1k_indel.hip"], cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    kernels = kernel_metadata(open(out).read())
    for pattern in (r"_Z7k_indelILb0EE", r"_Z7k_indelILb1EE"):
        mine = [k for k in kernels if re.match(pattern, k)]
        assert len(mine) == 1, (pattern, sorted(kernels))
        k = kernels[mine[0]]
        print("%s: %s VGPRs, %s SGPRs, %s + %s spilled, %s bytes of scratch" % (mine[0], k[".vgpr_count"], k[".sgpr_count"], k[".vgpr_spill_count"], k[".sgpr_spill_count"],
                                                                                k[".private_segment_fixed_size"]))
        assert int(k[".private_segment_fixed_size"]) == 0 and int(k[".group_segment_fixed_size"]) == 0, (mine[0], k)
        assert int(k[".vgpr_spill_count"]) == 0 and int(k[".sgpr_spill_count"]) == 0, (mine[0], k)


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def test_the_two_restatements_agree(table, want):
    other = ref.restate_by_regex(*ref.args(table))
    assert len(want.ev) > 3000 and want.ev == other.ev and ref.stats(want) == ref.stats(other) and want.trace == other.trace
    small = ref.generate(seed=7, records=300)
    a, b = ref.restate(*ref.args(small)), ref.restate_by_regex(*ref.args(small))
    assert a.ev == b.ev and ref.stats(a) == ref.stats(b) and a.events > 100
    # by hand: one string, every kind of run
    ops = [2, 2, 0, 3, 0, 2, 3, 3, 0, 3]
    assert ref.runs_by_loops(ops) == ref.runs_by_regex(ops) == [(2, 0, 2, 0, 0), (3, 3, 1, 1, 3), (2, 5, 1, 3, 4), (3, 6, 2, 3, 5), (3, 9, 1, 6, 6)]


def test_keys_round_trip(want):
    keys, counts = ref.expected_runs(want)
    assert keys == sorted(set(keys)) and min(counts) > 0 and max(keys) < 2 ** 63
    assert ref.from_runs(keys, counts) == want.ev
    assert {(k >> 29) & 3 for k in keys} == {0, 1, 2} and {k & 1 for k in keys} == {0, 1} and {(k >> 1) & 1 for k in keys} == {0, 1}
    # by hand: a deletion of 3 at g = 5 on the reverse strand, two uniq bookings and one other; CA inserted at g = 7; a long insertion of 14
    d = ((((5 << 2 | 0) << 27 | 3) << 1 | 1) << 1)
    i = ((((7 << 2 | 1) << 27 | (1 << 4 | 1 << 2 | 0)) << 1 | 0) << 1)
    l = ((((7 << 2 | 2) << 27 | 14) << 1 | 0) << 1)
    assert ref.key_of(5, 0, 3, 1, 1) == d and ref.key_of(5, 0, 3, 1, 0) == d + 1 and ref.key_of(7, 1, ref.payload_of(b"CA")[1], 0, 1) == i
    ev = ref.from_runs([d, d + 1, i + 1, l], [2, 1, 4, 1])
    assert ev == {(5, 0, 3, 1): [3, 2], (7, 1, 0b10100, 0): [4, 0], (7, 2, 14, 0): [1, 1]}
    assert ref.payload_of(b"ACGTACGTACGTA") == (1, (1 << 26) | int("0123012301230", 4)) and ref.payload_of(b"ACGTACGTACGTAC") == (2, 14) and ref.payload_of(b"AN") == (2, 2)
    assert ref.seq_of(ref.payload_of(b"ACGTACGTACGTA")[1]) == b"ACGTACGTACGTA" and ref.seq_of(ref.payload_of(b"T")[1]) == b"T"
    rows = ref.lines(ev, [0, 6, 20], ["ACGTAC", "GGGGGGGGGGGGGG"], min_count=1)
    assert rows == {(0, 6, 0, 3, "C"): (3, 2, 0, 3), (1, 1, 1, 2, "CA"): (4, 0, 4, 0), (1, 1, 1, 14, "*"): (1, 1, 1, 0)}
    assert list(ref.lines(ev, [0, 6, 20], ["ACGTAC", "GGGGGGGGGGGGGG"], min_count=4)) == [(1, 1, 1, 2, "CA")]


def test_normalisation_keeps_the_sequence_and_is_leftmost():
    rng = np.random.default_rng(11)
    moved = stopped_by_n = 0
    for _ in range(3000):
        n = int(rng.integers(2, 40))
        allele = bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), n, p=[0.4, 0.3, 0.15, 0.1, 0.05]))  # (skewed: repeats are frequent)
        length = int(rng.integers(1, 6))
        if rng.random() < 0.5 and n > length:
            p = int(rng.integers(0, n - length + 1))
            q = ref.normalise_del(allele, p, length)
            assert allele[:q] + allele[q + length:] == allele[:p] + allele[p + length:]
            assert q == 0 or allele[q - 1] != allele[q + length - 1] or allele[q - 1] == N
        else:
            p = int(rng.integers(0, n + 1))
            s = bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), length, p=[0.4, 0.3, 0.15, 0.1, 0.05]))
            q, z = ref.normalise_ins(allele, p, s)
            assert len(z) == length and allele[:q] + z + allele[q:] == allele[:p] + s + allele[p:]
            assert q == 0 or allele[q - 1] != z[-1] or z[-1] == N
            stopped_by_n += q > 0 and q < p and allele[q - 1] == N
        assert q <= p
        moved += q < p
    assert moved > 500 and stopped_by_n > 5


def test_table_covers_the_cases(table, want):
    assert table.allele_len == [63, 64, 65, 140, 1000, 4097] and table.records == 6000 and table.designed == 6000
    allele_of = table.aln["allele"].astype(np.int64)
    n_ops = table.aln["n_ops"].astype(np.int64)
    tr = want.trace                                                  # (record, first column, columns, op, p, normalised p, normalised S or None)
    ends = {(c + n) for _, c, n, _, _, _, _ in tr}
    # a run ending at column 63, one ending at column 64, one starting at column 64; a run that spans a whole step
    assert sum(1 for e in tr if e[1] + e[2] == 64) > 5 and sum(1 for e in tr if e[1] + e[2] == 65) > 5 and sum(1 for e in tr if e[1] == 64) > 5
    assert 128 in ends and 129 in ends
    assert any(n > 64 and c // 64 + 1 < (c + n) // 64 for _, c, n, _, _, _, _ in tr)
    assert {op for _, c, n, op, _, _, _ in tr if n > 64} == {2, 3}
    # two and three events (and many more) detected in one step: an event is detected at the column behind its run
    per_step = {}
    for e in tr:
        per_step[(e[0], (e[1] + e[2]) // 64)] = per_step.get((e[0], (e[1] + e[2]) // 64), 0) + 1
    assert {1, 2, 3} <= set(per_step.values()) and max(per_step.values()) >= 10
    # an insertion run touching a deletion run, in both orders
    behind = {(e[0], e[1] + e[2]): e[3] for e in tr}
    touching = {(e[3], behind[(e[0], e[1])]) for e in tr if (e[0], e[1]) in behind}
    assert touching == {(2, 3), (3, 2)}
    # runs at column 0 and at the last column, an edit string that is one gap run only: edge runs, no event
    first = table.ops[table.aln["ops_at"].astype(np.int64)]
    last = table.ops[table.aln["ops_at"].astype(np.int64) + n_ops - 1]
    assert ((first == 2).sum() > 20 and (first == 3).sum() > 20 and (last == 2).sum() > 20 and (last == 3).sum() > 20)
    whole = [i for i in range(len(table.aln)) if n_ops[i] > 1 and len(set(table.ops[int(table.aln["ops_at"][i]):int(table.aln["ops_at"][i]) + int(n_ops[i])].tolist())) == 1
             and first[i] in (2, 3)]
    assert {int(first[i]) for i in whole} == {2, 3} and not {e[0] for e in tr} & set(whole)
    assert all(e[1] > 0 and e[1] + e[2] < n_ops[e[0]] for e in tr) and want.edge_del > 100 and want.edge_ins > 100
    # insertions of 13 and of 14 bases: the last short key and the first long one
    ins = [e for e in tr if e[3] == 2]
    assert any(len(e[6]) == 13 and N not in e[6] for e in ins) and any(len(e[6]) == 14 for e in ins)
    types = {k[1] for k in want.ev}
    assert types == {0, 1, 2} and any(k[1] == 2 and k[2] <= 13 for k in want.ev) and any(k[1] == 2 and k[2] == 14 for k in want.ev)
    assert any(k[1] == 1 and k[2] >> 26 == 1 for k in want.ev)
    # an insertion containing N, and one whose shift an N of the allele stops
    ref_text = ref.reduce(table.allele_text)
    off = table.allele_off.astype(np.int64)
    assert any(N in e[6] for e in ins)
    assert any(e[5] < e[4] and e[5] > 0 and ref_text[int(off[allele_of[e[0]]]) + e[5] - 1] == N for e in ins)
    # a shift that reaches p == 0, by an insertion and by a deletion; a shift longer than the insertion
    assert any(e[5] == 0 and e[4] > 0 for e in ins) and any(e[5] == 0 and e[4] > 0 for e in tr if e[3] == 3)
    assert any(e[4] - e[5] > e[2] for e in ins) and any(e[4] - e[5] == e[2] for e in ins)
    assert want.shifted > 300 and want.events - want.shifted > 300
    # records with 0, 1 and several bookings, of both uniq values and both strands -- with events
    n_book = np.diff(table.book_ptr.astype(np.int64))
    with_events = np.zeros(len(table.aln), bool)
    with_events[[e[0] for e in tr]] = True
    assert set(np.unique(n_book[with_events])) >= {0, 1, 2, 3, 4, 5, 256} and (n_book[with_events] == 0).sum() > 100
    assert set(np.unique(table.strand[with_events])) == {0, 1} and set(np.unique(table.book_uniq)) == {0, 1}
    assert any(0 < u < n for n, u in want.ev.values())
    # the same indel placed at several offsets of one repeat by different records: one key
    g0 = int(off[3])
    raw = {e[4] for e in tr[:] if allele_of[e[0]] == 3 and e[3] == 3 and e[2] == 1 and e[0] >= table.designed and e[5] == ref.HOMOPOLYMER[0]}
    assert raw == set(range(*ref.HOMOPOLYMER))
    there = [k for k in want.ev if k[0] == g0 + ref.HOMOPOLYMER[0] and k[1] == 0 and k[2] == 1]
    assert 1 <= len(there) <= 2 and sum(want.ev[k][0] for k in there) >= 8           # (one key per strand)
    assert not [k for k in want.ev if g0 + ref.HOMOPOLYMER[0] < k[0] < g0 + ref.HOMOPOLYMER[1] and k[1] == 0 and k[2] == 1]
    ca = [e for e in tr if allele_of[e[0]] == 3 and e[0] >= table.designed and e[3] == 2 and e[6] == b"CA" and e[5] == ref.DINUCLEOTIDE[0]]
    assert {e[4] for e in ca} == set(range(ref.DINUCLEOTIDE[0], ref.DINUCLEOTIDE[1] + 1))
    # the keys the kernel emits
    emitted = sum(v[0] for v in want.ev.values())
    assert 20000 <= emitted <= 2000000 and want.events > 10000


def test_table_text_round_trip(tmp_path):
    ev = {(2, 0, 2, 0): [3, 1], (2, 0, 2, 1): [1, 1], (2, 1, ref.payload_of(b"GT")[1], 0): [2, 0], (0, 1, ref.payload_of(b"A")[1], 1): [1, 0], (9, 2, 20, 0): [5, 5],
          (9, 1, ref.payload_of(b"T")[1], 0): [1, 0], (9, 0, 1, 0): [1, 0]}
    names, seqs, masks = ["X*01", "Y*02"], ["ACGTAC", "TTNGG"], [[1, 1, 0, 1, 1, 1], [0, 1, 1, 1, 0]]
    rows = ref.lines(ev, [0, 6, 11], seqs)
    assert rows[(0, 3, 0, 2, "GT")] == (4, 2, 3, 1) and rows[(0, 0, 1, 1, "A")] == (1, 0, 0, 1)
    p = tmp_path / "t.tsv"
    p.write_text(ref.table_text(names, seqs, masks, rows))
    header, got = ref.parse(str(p))
    assert header == ref.HEADER
    # by allele, pos, DEL before INS, len, seq; exon_pos '.' for pos 0 and outside exons
    assert [r[:6] for r in got] == [("X*01", 0, None, "INS", 1, "A"), ("X*01", 2, 2, "INS", 2, "GT"), ("X*01", 3, None, "DEL", 2, "GT"), ("Y*02", 3, 2, "INS", 1, "T"),
                                    ("Y*02", 3, 2, "INS", 20, "*"), ("Y*02", 4, 3, "DEL", 1, "G")]
    assert got[2][6] == dict(zip(ref.COLUMNS, (4, 2, 3, 1)))
    assert [r[:2] for r in ref.parse_text_rows(ref.table_text(names, seqs, masks, ref.lines(ev, [0, 6, 11], seqs, min_count=4)))] == [("X*01", 3), ("Y*02", 3)]


def test_analyzer_records():
    import pileup_ref
    ptr, asg, ops = pileup_ref.assignments([
        [(0, pileup_ref.overlap(0, 1, 4, 2, 5, -1), [0, 0, 1, 0], pileup_ref.overlap(0, 0, 2, 7, 9), [0, 0, 0])],
        [(0, pileup_ref.overlap(0, 0, 3, 0, 3), [0] * 4), (1, pileup_ref.overlap(1, 0, 3, 1, 4, -1), [0] * 4, None, [], 1)]])
    aln, text, strand, book_ptr, book_uniq = ref.analyzer_records(ptr, asg, ["ACGTA", "ACGT"], ["TTT", "GGGG"])
    assert len(aln) == 4 and book_ptr.tolist() == [0, 1, 2, 3, 4] and strand.tolist() == [1, 0, 0, 1] and book_uniq.tolist() == [1, 1, 0, 0]
