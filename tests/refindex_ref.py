"""The reference index t1k_ref_upload builds, restated plainly (no GPU, no packed-word arithmetic): an allele-by-allele, position-by-
position loop like KmerIndex::BuildIndexFromRead (KmerIndex.hpp:107-130) over KmerCode's rules (KmerCode.hpp:93-108), laid out as the
comments of T1kRefDev (t1k_amd/csrc/t1k_dev.h) and of t1k_ref_upload (t1k_amd/csrc/t1k_refindex.hip) say.

A k-mer's code holds its FIRST base in the lowest two bits (the device's order; the reference and the oracle put it in the highest):
code = sum of base[j] * 4^j.  Letters outside ACGT are N: they make the windows that hold them invalid and contribute n_base_code.

`mutation` builds a deliberately wrong index (MUTATIONS): tests/test_refindex_cpu.py shows that the designed cases tell each of them
from the right one."""
import bisect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = {"A": 0, "C": 1, "G": 2, "T": 3}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
MUTATIONS = ("no_i_eq_k",            # the `i == k` clause of KmerIndex.hpp:121 left out
             "prev_if_valid",        # the previous window compared only when it was valid
             "first_vs_nothing",     # the first window compared with nothing (always inserted when valid)
             "sort_offset_first",    # a list ordered by offset, then allele
             "dir_bound_le",         # directory cell = postings with allele <= the chunk's first, instead of <
             "mask_no_guard",        # mask bit of chunk c without `c + 1 < stride`: reads the cells behind the row
             "multi_first_two",      # kMulti from the first two postings only
             "n_ignored_last_base")  # the N mask not looked at for the window's last base


def constants():
    """T1K_DIR_MINLEN, T1K_SEED_CHUNK, T1K_NO_DIR as t1k_dev.h defines them"""
    text = open(os.path.join(ROOT, "t1k_amd", "csrc", "t1k_dev.h")).read()
    out = {}
    for name in ("T1K_DIR_MINLEN", "T1K_SEED_CHUNK", "T1K_NO_DIR"):
        m = re.findall(r"^\s*#define\s+%s\s+(0x[0-9A-Fa-f]+|\d+)u?\b" % name, text, re.M)
        assert len(m) == 1, name
        out[name] = int(m[0], 0)
    return out


def encode(text):
    """the device's code of a k-mer text over ACGT"""
    return sum(BASE[c] << (2 * j) for j, c in enumerate(text))


def decode(code, k):
    return "".join("ACGT"[(code >> (2 * j)) & 3] for j in range(k))


def revcomp(text):
    return "".join(COMP[c] for c in reversed(text))


def canonical_prefix(code, k):
    """the first kp = max(1, k - 2) bases of the smaller of (code, code of the reverse complement), as a code"""
    t = decode(code, k)
    r = encode(revcomp(t))
    return encode(decode(min(code, r), k)[:max(1, k - 2)])


def windows(seq, k, n_code, mutation=None):
    """[(offset, code, valid, inserted)] of every window of one allele, by the loop of BuildIndexFromRead: i is the window's last base"""
    out = []
    prev = None
    for i in range(k - 1, len(seq)):
        w = seq[i - k + 1:i + 1]
        code = sum(BASE.get(c, n_code) << (2 * j) for j, c in enumerate(w))
        valid = all(c in BASE for c in (w[:-1] if mutation == "n_ignored_last_base" else w))
        if i == k - 1:
            before = None if mutation == "first_vs_nothing" else 0  # prevKmerCode starts as code 0
        elif mutation == "prev_if_valid" and not prev[1]:
            before = None
        else:
            before = prev[0]  # whatever its validity
        second = i == k and mutation != "no_i_eq_k"
        out.append((i - k + 1, code, valid, valid and (second or code != before)))
        prev = (code, valid)
    return out


def _pack(values, shift_bits=2):
    """per-position values (uint64, a multiple of 32 of them) -> words, position q of a word at bit 2q"""
    v = np.asarray(values, np.uint64).reshape(-1, 32)
    sh = (np.arange(32, dtype=np.uint64) * np.uint64(shift_bits))
    return np.bitwise_or.reduce(v << sh, axis=1)


class Index:
    """everything t1k_ref_upload leaves on the device.  Small arrays are attributes; the arrays of 4^k cells are made by dense() (k <= 12)
    or read cell by cell (k_start, dir_idx, has_word ...), which is all a k = 15 case can afford."""

    def __init__(self, seqs, k, n_code, exon=None, mutation=None, transpose=True):
        cst = constants()
        self.MINLEN, self.CHUNK, self.NO_DIR = cst["T1K_DIR_MINLEN"], cst["T1K_SEED_CHUNK"], cst["T1K_NO_DIR"]
        self.k, self.n_code, self.seqs = k, n_code, list(seqs)
        A = len(seqs)
        assert A > 0
        # layout: every allele on a 32-base boundary with at least one spare position behind it
        self.alleleLen = np.array([len(s) for s in seqs], np.uint32)
        off, total = [], 0
        for s in seqs:
            off.append(total)
            total += (len(s) + 32) // 32 * 32
        total += 64
        self.alleleOff = np.array(off, np.uint64)
        self.totalBases = total
        self.nWords = total // 32 + 2
        npos = self.nWords * 32
        base, nflag, ex, posted = (np.zeros(npos, np.uint64) for _ in range(4))
        sep_start, sep_pos, has_n = [0], [], []
        self.lists = {}      # code -> [(allele, offset)] in insertion order
        self.seen = set()    # the code of every window, valid or not
        for a, s in enumerate(seqs):
            g = off[a]
            for i, c in enumerate(s):
                if c in BASE:
                    base[g + i] = BASE[c]
                else:
                    base[g + i] = n_code
                    nflag[g + i] = 1
                    sep_pos.append(i)
                if exon is not None and exon[a][i]:
                    ex[g + i] = 1
            sep_start.append(len(sep_pos))
            has_n.append(1 if sep_start[-1] > sep_start[-2] else 0)
            for o, code, valid, ins in windows(s, k, n_code, mutation):
                self.seen.add(code)
                if ins:
                    self.lists.setdefault(code, []).append((a, o))
                    posted[g + o] = 1
        if mutation == "sort_offset_first":
            for l in self.lists.values():
                l.sort(key=lambda p: (p[1], p[0]))
        self.bases, self.nmask, self.exon, self.posted = _pack(base), _pack(nflag), _pack(ex), _pack(posted)
        self.sepStart = np.array(sep_start, np.uint32)
        self.sepPos = np.array(sep_pos, np.int32)
        self.alleleHasN = np.array(has_n, np.uint8)
        # postings: lists by ascending code, each in its own order
        self.codes = sorted(self.lists)
        self.starts = [0]
        for c in self.codes:
            self.starts.append(self.starts[-1] + len(self.lists[c]))
        self.nPost = self.starts[-1]
        flat = [p for c in self.codes for p in self.lists[c]]
        self.kPost = np.array(flat, np.uint32).reshape(-1, 2)
        self.kPostAllele = self.kPost[:, 0].copy()
        # bitmaps
        self.multi = set()
        for c, l in self.lists.items():
            al = [a for a, _ in l]
            if (len(l) > 1 and al[0] == al[1]) if mutation == "multi_first_two" else (len(set(al)) < len(al)):
                self.multi.add(c)
        self.pre = set(canonical_prefix(c, k) for c in self.codes)
        # chunk directory: one row per list longer than MINLEN, rows by ascending code
        self.rowCodes = [c for c in self.codes if len(self.lists[c]) > self.MINLEN]
        self.rowOf = {c: r for r, c in enumerate(self.rowCodes)}
        self.dirRows = len(self.rowCodes)
        self.stride = (A + self.CHUNK - 1) // self.CHUNK + 1
        self.maskWords = max(1, (self.stride - 1 + 63) // 64)
        cells = []
        for c in self.rowCodes:
            al = [a for a, _ in self.lists[c]]
            for ci in range(self.stride):
                bound = ci * self.CHUNK
                cells.append(sum(1 for a in al if (a <= bound if mutation == "dir_bound_le" else a < bound)))
        self.kDir = np.array(cells, np.uint32)
        masks = []
        for r in range(self.dirRows):
            for w in range(self.maskWords):
                m = 0
                for b in range(64):
                    ci = 64 * w + b
                    if mutation == "mask_no_guard":
                        at = r * self.stride + ci
                        d0, d1 = (cells[at] if at < len(cells) else 0), (cells[at + 1] if at + 1 < len(cells) else 0)
                        if d1 > d0:
                            m |= 1 << b
                    elif ci + 1 < self.stride and cells[r * self.stride + ci + 1] > cells[r * self.stride + ci]:
                        m |= 1 << b
                masks.append(m)
        self.kDirMask = np.array(masks, np.uint64)
        # transposed copy: blocks of 64 consecutive alleles, as many rows of 64 words as the block's longest allele has words, plus 2;
        # 512 zero words behind the last block
        nb = (A + 63) // 64
        block, tt = [], 0
        for b in range(nb):
            words = max((len(s) + 31) // 32 for s in seqs[b * 64:b * 64 + 64])
            block.append(tt)
            tt += (words + 2) * 64
        self.hasT = bool(transpose) and tt + 512 < (1 << 32)
        if self.hasT:
            self.blockT = np.array(block, np.uint32)
            t = np.zeros(tt + 512, np.uint64)
            for a, s in enumerate(seqs):
                for w in range((len(s) + 31) // 32):
                    t[block[a >> 6] + w * 64 + (a & 63)] = self.bases[off[a] // 32 + w]
            self.basesT = t
        else:
            self.blockT, self.basesT = np.zeros(0, np.uint32), np.zeros(0, np.uint64)

    # ---- cell by cell ----
    def list_of(self, code):
        return self.lists.get(code, [])

    def k_start(self, c):
        """kStart[c] = postings of the codes below c, for c = 0 .. 4^k"""
        return self.starts[bisect.bisect_left(self.codes, c)]

    def dir_idx(self, c):
        return self.rowOf.get(c, self.NO_DIR)

    def _word(self, members, w):
        return sum(1 << b for b in range(32) if 32 * w + b in members)

    def has_word(self, w):
        return self._word(self.lists, w)

    def multi_word(self, w):
        return self._word(self.multi, w)

    def pre_word(self, w):
        return self._word(self.pre, w)

    # ---- whole arrays ----
    def _bitmap(self, members, n):
        out = np.zeros((n + 31) // 32, np.uint32)
        for c in members:
            out[c >> 5] |= np.uint32(1 << (c & 31))
        return out

    def small(self):
        """the arrays whose size does not grow with 4^k, by their names in t1k_amd.REF_ARRAYS"""
        return dict(bases=self.bases, nmask=self.nmask, exon=self.exon, posted=self.posted, basesT=self.basesT, blockT=self.blockT, alleleOff=self.alleleOff,
                    alleleLen=self.alleleLen, alleleHasN=self.alleleHasN, sepStart=self.sepStart, sepPos=self.sepPos, kDir=self.kDir, kDirMask=self.kDirMask,
                    kPost=self.kPost, kPostAllele=self.kPostAllele)

    def dense(self):
        """the arrays of 4^k cells"""
        n = 1 << (2 * self.k)
        assert self.k <= 12
        cnt = np.zeros(n + 1, np.uint32)
        for c, l in self.lists.items():
            cnt[c] = len(l)
        k_start = np.zeros(n + 1, np.uint32)
        k_start[1:] = np.cumsum(cnt[:-1], dtype=np.uint64)
        idx = np.full(n, self.NO_DIR, np.uint32)
        for c, r in self.rowOf.items():
            idx[c] = r
        return dict(kStart=k_start, kHas=self._bitmap(self.lists, n), kMulti=self._bitmap(self.multi, n),
                    kHasPre=self._bitmap(self.pre, 1 << (2 * max(1, self.k - 2))), kDirIdx=idx)

    def geometry(self):
        return dict(n_alleles=len(self.seqs), k=self.k, total_bases=self.totalBases, n_words=self.nWords, n_postings=self.nPost, bases_t_len=len(self.basesT),
                    n_sep=len(self.sepPos), dir_rows=self.dirRows, dir_stride=self.stride, dir_mask_words=self.maskWords, has_bases_t=1 if self.hasT else 0)

    def fingerprint(self):
        """what two builds are compared by (the mutation test): every array's bytes, the big ones through their members"""
        s = self.small()
        return {**{n: a.tobytes() for n, a in s.items()}, "lists": sorted((c, tuple(l)) for c, l in self.lists.items()), "multi": sorted(self.multi),
                "pre": sorted(self.pre), "rows": tuple(self.rowCodes)}


def build(seqs, k, n_code, exon=None, mutation=None, transpose=True):
    assert mutation is None or mutation in MUTATIONS
    return Index(seqs, k, n_code, exon, mutation, transpose)
