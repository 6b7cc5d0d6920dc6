"""CPU tests (no GPU) of the analyzer's SAM output (--sam): the usage text, the header-only file of an empty selection, and
the restatement tests/sam_ref.py itself -- hand-worked CIGAR and MD strings, the round trip through the independent decoder, the byte
bounds of include/t1k_gpu.h."""
import os
import subprocess

import numpy as np
import pytest

import sam_ref as ref
import util

ANALYZER = os.path.join(util.ROOT, "t1k_amd", "bin", "analyzer")
ALLELE = "ACGTTGCANACGT"      # position: A0 C1 G2 T3 T4 G5 C6 A7 N8 A9 C10 G11 T12


def test_usage_names_the_flag(built):
    r = subprocess.run([ANALYZER], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "--sam" in r.stderr and "prefix_aligned.sam" in r.stderr
    lines = r.stderr.split("\n")
    at = [i for i, l in enumerate(lines) if l.startswith("\t--sam:")][0]
    assert "no counterpart in the reference" in lines[at] + lines[at + 1]


def test_empty_selection_gives_the_header_alone(built, tmp_path):
    ref_fa, empty, out = tmp_path / "ref.fa", tmp_path / "none.tsv", str(tmp_path / "o")
    ref_fa.write_text(">A*01\nACGT\n")
    empty.write_text("")
    r = subprocess.run([ANALYZER, "-f", str(ref_fa), "-a", str(empty), "-u", str(ref_fa), "-o", out, "--sam"], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert open(out + "_aligned.sam").read() == ref.HD + "\n" + ref.PG + "\n"
    r = subprocess.run([ANALYZER, "-f", str(ref_fa), "-a", str(empty), "-u", str(ref_fa), "-o", out + "2"], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and not os.path.exists(out + "2_aligned.sam")


HAND = [
    # ops, seq_start, clip -> cigar, md, nm, span
    ([0, 0, 1, 0], 0, (0, 0), "4M", "2G1", 1, 4),
    ([1, 0, 0, 0], 0, (0, 0), "4M", "0A3", 1, 4),                      # mismatch first
    ([0, 0, 0, 1], 0, (0, 0), "4M", "3T0", 1, 4),                      # ... last
    ([1, 0, 0, 1], 1, (0, 0), "4M", "0C2T0", 2, 4),                    # ... both
    ([0, 1, 1, 0], 0, (0, 0), "4M", "1C0G1", 2, 4),                    # two adjacent mismatches
    ([3, 0, 0], 0, (0, 0), "1D2M", "0^A2", 1, 3),                      # deletion first
    ([0, 0, 3], 0, (0, 0), "2M1D", "2^G0", 1, 3),                      # ... last
    ([0, 1, 3, 3, 0], 0, (0, 0), "2M2D1M", "1C0^GT1", 3, 5),           # ... after a mismatch
    ([0, 3, 1, 0], 0, (0, 0), "1M1D2M", "1^C0G1", 2, 4),               # mismatch after a deletion: the 0 keeps them apart
    ([3, 2, 3], 0, (0, 0), "1D1I1D", "0^A0^C0", 3, 2),                 # an insert ends a deletion run
    ([3, 3, 3], 5, (0, 0), "3D", "0^GCA0", 3, 3),
    ([2, 2, 2], 0, (0, 0), "3I", "0", 3, 0),                           # all insert
    ([2, 2, 2], 13, (0, 0), "3I", "0", 3, 0),                          # ... behind the allele's last base
    ([0, 2, 2, 0], 0, (0, 0), "1M2I1M", "2", 2, 2),                    # inserts are invisible in MD
    ([2, 0, 0, 2], 0, (0, 0), "1I2M1I", "2", 2, 2),                    # runs are literal
    ([0, 0], 0, (3, 0), "3S2M", "2", 0, 2),                            # clips
    ([0, 0], 0, (0, 12), "2M12S", "2", 0, 2),
    ([0, 1], 11, (10, 100), "10S2M100S", "1T0", 1, 2),                 # ... and the allele's last position
    ([0, 1, 0], 7, (0, 0), "3M", "1N1", 1, 3),                         # N is copied as it stands
    ([0, 3, 0], 7, (0, 0), "1M1D1M", "1^N1", 1, 3),
    ([0] * 12, 0, (0, 0), "12M", "12", 0, 12),
]


@pytest.mark.parametrize("ops,start,clip,cigar,md,nm,span", HAND)
def test_hand_worked_strings(ops, start, clip, cigar, md, nm, span):
    assert ref.encode(ops, start, ALLELE, clip) == (cigar, md, nm, span)
    n_read = sum(1 for o in ops if o != 3)
    seq = "".join("x" for _ in range(clip[0])) + "".join("acgt"[i % 4] for i in range(n_read)) + "".join("x" for _ in range(clip[1]))
    got, bases = ref.decode(cigar, md, seq)
    assert got == list(ops) and len(bases) == span


def test_encode_refuses_what_the_kernel_refuses():
    for bad in (lambda: ref.encode([0, 4], 0, ALLELE), lambda: ref.encode([], 0, ALLELE), lambda: ref.encode([0, 0], 12, ALLELE), lambda: ref.encode([3], 13, ALLELE)):
        with pytest.raises(ValueError):
            bad()


def _random_case(rng):
    n = int(rng.integers(1, 200))
    p = [(0.85, 0.05, 0.05, 0.05), (0.25, 0.25, 0.25, 0.25), (0.5, 0.0, 0.25, 0.25)][int(rng.integers(0, 3))]
    ops = rng.choice(4, n, p=p)
    span = int((ops != 2).sum())
    allele = "".join("ACGTN"[i] for i in rng.choice(5, span + int(rng.integers(0, 5)) + 1, p=[0.24, 0.24, 0.24, 0.24, 0.04]))
    start = int(rng.integers(0, len(allele) - span + 1))
    clip = (int(rng.choice([0, 0, 3, 10])), int(rng.choice([0, 0, 7, 100])))
    return ops, start, allele, clip


def test_round_trip_and_bounds_on_random_strings():
    rng = np.random.default_rng(5)
    for _ in range(5000):
        ops, start, allele, clip = _random_case(rng)
        cigar, md, nm, span = ref.encode(ops, start, allele, clip)
        # the read that these columns describe: the allele's base on a match, another base on a mismatch, anything on an insert
        seq, t = ["x"] * clip[0], start
        for o in ops:
            if o == 0:
                seq.append(allele[t])
            elif o == 1:
                seq.append("a" if allele[t] != "A" else "c")
            elif o == 2:
                seq.append("g")
            t += 1 if o != 2 else 0
        seq += ["x"] * clip[1]
        got, bases = ref.decode(cigar, md, "".join(seq))
        assert got == ops.tolist() and bases == allele[start:start + span], (ops, cigar, md)
        assert nm == int((ops != 0).sum()) and span == int((ops != 2).sum())
        assert len(cigar) <= 2 * len(ops) + 22 and len(md) <= 3 * len(ops) + 11


def test_byte_bounds_at_the_alternating_strings():
    """the bounds of include/t1k_gpu.h, at the strings its derivation names.  CIGAR: 2 * n_ops + 22 is attained (every run one column, two
    clips of ten digits).  MD: 3 * n_ops + 11 holds and is NOT tight -- a deletion column costs the 3 bytes of the derivation (0^C), but
    two deletion runs need a column between them, and the dearest one is a mismatch (2 bytes): 2.5 * n_ops + 1 for `3 1` alternating,
    1.5 * n_ops + 1 for `3 2`, 3 * n_ops + 1 for the single column."""
    allele = "ACGT" * 64
    n = 128
    for a, b in ((0, 2), (0, 3), (2, 3), (3, 2), (1, 2)):
        cigar, md, _, _ = ref.encode([a, b] * 64, 0, allele, (4294967295, 4294967295))
        assert len(cigar) == 2 * n + 22, (a, b)
        assert len(md) <= 3 * n + 11
    assert len(ref.encode([3, 2] * 64, 0, allele)[1]) == 3 * 64 + 1 and ref.encode([3, 2] * 2, 0, allele)[1] == "0^A0^C0"
    assert len(ref.encode([0, 3] * 64, 0, allele)[1]) == 3 * 64 + 1 and ref.encode([0, 3] * 2, 0, allele)[1] == "1^C1^T0"
    assert len(ref.encode([3, 1] * 64, 0, allele)[1]) == 5 * 64 + 1
    assert ref.encode([3], 0, allele) == ("1D", "0^A0", 1, 1) and len("0^A0") == 3 * 1 + 1
    cigar, md, _, _ = ref.encode([0] * 1000, 0, "A" * 1000)
    assert (cigar, md) == ("1000M", "1000")


def test_pileup_from_sam_books_what_the_walk_books():
    import pileup_ref
    ptr, asg, ops, r1, r2, allele_len = pileup_ref.random_assignments(3, fragments=120)
    rng = np.random.default_rng(9)
    seqs = ["".join("ACGT"[i] for i in rng.integers(0, 4, n)) for n in allele_len]
    names = ["a%d" % i for i in range(len(seqs))]
    lines = ref.header(names, seqs) + ref.sam_lines(names, seqs, ["f%d" % f for f in range(len(ptr) - 1)], ptr, asg, ops, r1, r2)
    assert np.array_equal(ref.pileup_from_sam(lines), pileup_ref.restate_by_loops(ptr, asg, ops, r1, r2, allele_len))
    recs = [ref.parse_line(l) for l in lines if not l.startswith("@")]
    assert len(recs) == int((asg["has_mate_pair"] != 0).sum()) + len(asg)
    for r in recs:                                    # every line decodes to an edit string of its own length
        got, bases = ref.decode(r["cigar"], r["tags"]["MD"], r["seq"])
        assert sum(1 for o in got if o != 0) == r["tags"]["NM"] and len(r["seq"]) == 60
