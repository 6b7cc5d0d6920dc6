#!/usr/bin/env python3
"""Writes a UMI file for a barcode file, for measuring analyzer --umi at size.

    python tools/umi_at_size.py BARCODES.fa OUT_umi.fa [--seed 1] [--dup 0.333] [--err 0.01] [--len 12]

One record per record of BARCODES.fa, under the same name, in the same order.  About --dup of the fragments repeat the UMI of the previous
fragment of their barcode (PCR duplicates: the analyzer collapses those that also share the gene), the others draw a new one; --err of all
of them then get one base changed (sequencing errors: --umiMismatch 1 joins them to their source where that is at least twice as frequent)."""
import argparse

import numpy as np


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("barcodes")
    ap.add_argument("out")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dup", type=float, default=1.0 / 3)
    ap.add_argument("--err", type=float, default=0.01)
    ap.add_argument("--len", type=int, default=12)
    a = ap.parse_args()
    if not 1 <= a.len <= 16:
        ap.error("--len takes 1 .. 16")
    lines = open(a.barcodes, "rb").read().split(b"\n")
    names, bcs = lines[0::2], lines[1::2]
    n = min(len(names), len(bcs))
    while n and not names[n - 1]:
        n -= 1
    names, bcs = names[:n], bcs[:n]
    if any(not x.startswith(b">") for x in names[:1000]):
        raise SystemExit("umi_at_size: %s is not a two-line FASTA" % a.barcodes)
    rng = np.random.default_rng(a.seed)
    bc = np.unique(np.array(bcs), return_inverse=True)[1]
    order = np.argsort(bc, kind="stable")            # the fragments barcode by barcode, file order inside
    first = np.ones(n, bool)
    first[1:] = bc[order][1:] != bc[order][:-1]
    fresh = first | (rng.random(n) >= a.dup)         # draws a new UMI; the others repeat the last fresh one before them
    src = np.maximum.accumulate(np.where(fresh, np.arange(n), 0))
    code = rng.integers(0, 4 ** a.len, n)[src]
    err = rng.random(n) < a.err
    code[err] ^= (rng.integers(1, 4, n) << (2 * rng.integers(0, a.len, n)))[err]
    out = np.empty(n, np.int64)
    out[order] = code
    text = np.frombuffer(b"ACGT", np.uint8)[(out[:, None] >> (2 * np.arange(a.len - 1, -1, -1))) & 3]   # first base most significant
    with open(a.out, "wb") as f:
        step = 1 << 20
        for i in range(0, n, step):
            f.write(b"".join(nm.split()[0] + b"\n" + text[j].tobytes() + b"\n" for j, nm in enumerate(names[i:i + step], i)))
    print("umi_at_size: %d records, %d of them repeats, %d with an error -> %s" % (n, int((~fresh).sum()), int(err.sum()), a.out))


if __name__ == "__main__":
    main()
