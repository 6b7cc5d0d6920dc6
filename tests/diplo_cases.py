"""Inputs of the diplotype tests (t1k_diplo_batch, genotyper --diplotypes): tables of read groups over candidate ids that hold
every case the kernel can go wrong at, random small tables, the inputs the C ABI must refuse, and an allele-level input for the classes
and candidates the host forms.  Shared by test_diplo_cpu.py and test_gpu_diplo.py."""
import numpy as np

SIZES = (1, 2, 63, 64, 65, 128, 129, 257)


class Case:
    """the arguments of t1k_diplo_batch"""

    def __init__(self, groups, q, counts):
        self.groups = [sorted(int(a) for a in g) for g in groups]
        self.group_ptr = np.concatenate([[0], np.cumsum([len(g) for g in self.groups])]).astype(np.uint64)
        self.ent = np.array([a for g in self.groups for a in g], dtype=np.uint32)
        self.q = np.array(q, dtype=np.uint64)
        self.cand_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
        assert len(self.q) == len(self.groups) and all(len(set(g)) == len(g) for g in self.groups)
        for a in (self.group_ptr, self.ent, self.q, self.cand_ptr):
            a.setflags(write=False)

    def args(self):
        return self.group_ptr, self.ent, self.q, self.cand_ptr

    def ids(self, gene):
        return list(range(int(self.cand_ptr[gene]), int(self.cand_ptr[gene + 1])))


# candidates per gene of designed(): gene 1 has a single candidate, no group holds gene 2, gene 3 has none at all
COUNTS = (70, 1, 30, 0, 100, 130, 60)


def designed(seed=7):
    """Groups of every size in SIZES drawn over all genes but gene 2 (three of each), and by hand:
    ends_at_63     64 ids of gene 4, then 30 of gene 5: one segment ends at lane 63, the next begins at lane 64;
    straddles      40 ids of gene 0, then 60 of gene 4 (positions 40 .. 99), then 50 of gene 5: segments across the 64-boundaries of a long list;
    all_of_gene_0  the 70 candidates of gene 0 and nothing else;
    all_of_0_and_1 the same with the single candidate of gene 1 behind them;
    single         the candidate of gene 1 alone; with one neighbour of gene 0; with one of gene 4;
    whole_tiles    128 ids of gene 5 (a segment of exactly two tiles) and all 130 of them (two tiles and two ids)."""
    rng = np.random.default_rng(seed)
    c = Case([], [], COUNTS)
    gene = [c.ids(x) for x in range(len(COUNTS))]
    allowed = [i for x in (0, 1, 4, 5, 6) for i in gene[x]]
    groups, tags = [], []
    for n in SIZES:
        for _ in range(3):
            groups.append(rng.choice(allowed, size=n, replace=False).tolist())
            tags.append("size%d" % n)
    pick = lambda x, n: rng.choice(gene[x], size=n, replace=False).tolist()
    by_hand = {
        "ends_at_63": pick(4, 64) + pick(5, 30),
        "straddles": pick(0, 40) + pick(4, 60) + pick(5, 50),
        "all_of_gene_0": gene[0],
        "all_of_0_and_1": gene[0] + gene[1],
        "single": gene[1],
        "single_after_0": [gene[0][-1]] + gene[1],
        "single_before_4": gene[1] + [gene[4][0]],
        "two_tiles": pick(5, 128),
        "two_tiles_and_two": gene[5],
    }
    for name, g in by_hand.items():
        groups.append(g)
        tags.append(name)
    q = rng.integers(1, 1 << 22, size=len(groups)).tolist()
    q[3] = (1 << 40) + 12345
    q[17] = 1
    c = Case(groups, q, COUNTS)
    c.tags = tags
    return c


def adjacent_case(seed=3):
    """two genes (5 and 7 candidates, a gene without candidates between them) whose segments are adjacent in every group"""
    rng = np.random.default_rng(seed)
    groups = []
    for _ in range(40):
        a = rng.choice(5, size=int(rng.integers(1, 6)), replace=False).tolist()
        b = (5 + rng.choice(7, size=int(rng.integers(1, 8)), replace=False)).tolist()
        groups.append(a + b)
    return Case(groups, rng.integers(1, 1 << 30, size=len(groups)).tolist(), (5, 0, 7))


def hot_cell_case(n=20000):
    """n groups that hold the same pair of candidates, q near 2^40: every add lands on three cells and the sums pass 2^54"""
    q = (1 << 40) - np.arange(n, dtype=np.uint64) * np.uint64(3)
    return Case([[1, 2]] * n, q, (3,))


def random_case(seed, n_genes=4, per=6, n_groups=40, max_size=10):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, per + 1, size=n_genes).tolist()
    counts[int(rng.integers(0, n_genes))] = per
    total = sum(counts)
    groups = [rng.choice(total, size=int(rng.integers(1, min(max_size, total) + 1)), replace=False).tolist() for _ in range(n_groups)]
    return Case(groups, rng.integers(1, 1 << 24, size=n_groups).tolist(), counts)


def refusals():
    """name -> (expected code name, (group_ptr, ent, q, cand_ptr)); the sound input they are all one change away from is 'sound'"""
    gp = np.array([0, 3, 5], dtype=np.uint64)
    ent = np.array([0, 2, 3, 1, 2], dtype=np.uint32)
    q = np.array([5, 7], dtype=np.uint64)
    cp = np.array([0, 3, 4], dtype=np.uint32)

    def edit(a, i, v):
        b = a.copy()
        b[i] = v
        return b
    return {
        "sound": ("OK", (gp, ent, q, cp)),
        "ptr_start": ("ARG", (edit(gp, 0, 1), ent, q, cp)),
        "ptr_decreases": ("ARG", (np.array([0, 5, 3], dtype=np.uint64), ent, q, cp)),
        "cand_ptr_start": ("ARG", (gp, ent, q, edit(cp, 0, 1))),
        "cand_ptr_decreases": ("ARG", (gp, ent, q, np.array([0, 4, 3, 4], dtype=np.uint32))),
        "id_range": ("ARG", (gp, edit(ent, 4, 4), q, cp)),
        "duplicate": ("ARG", (gp, edit(ent, 1, 0), q, cp)),
        "descending": ("ARG", (gp, edit(ent, 3, 3), q, cp)),
        "gene_2049": ("CAPACITY", (gp, ent, q, np.array([0, 3, 2052], dtype=np.uint32))),
        "cells_2_29": ("CAPACITY", (gp, ent, q, (np.arange(130, dtype=np.uint32) * np.uint32(2048)))),   # 129 genes of 2048: 2^29 + 2^22 cells
        "sum_2_63": ("CAPACITY", (gp, ent, np.array([1 << 62, 1 << 62], dtype=np.uint64), cp)),
        "q_2_63": ("CAPACITY", (gp, ent, np.array([1 << 63, 0], dtype=np.uint64), cp)),
    }


# ---- allele level: what the host makes of a job's groups ---------------------------------------------------------------------------------
class HostCase:
    def __init__(self, holds, q, allele_gene, called):
        """holds: allele -> the groups that hold it"""
        G = len(q)
        rows = [sorted(a for a, gs in holds.items() if g in gs) for g in range(G)]
        assert all(rows), "every group holds an allele"
        self.group_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
        self.alleles = np.array([a for r in rows for a in r], dtype=np.uint32)
        self.q = np.array(q, dtype=np.uint64)
        self.allele_gene = np.array(allele_gene, dtype=np.uint32)
        self.called = list(called)

    def args(self):
        return self.group_ptr, self.alleles, self.q, self.allele_gene, self.called


def host_designed():
    """gene 0 (alleles 0 .. 49): a class of 40 (alleles 5 .. 44, groups 0 1 2) that holds the allele called in slot 0, 17 -- not its smallest
    index; alleles 0, 1 and 45 in groups 0 and 3, where 45 alone also lies in group 9, whose weight is 0: one class of three; a class of two
    (46, 47: group 5); single alleles 2, 3 and 4; slot 1 calls allele 3, the lightest class, so that 2 or 3 candidates must force it in; 48
    lies in no group and 49 only in group 9: neither takes part.
    gene 1 (50 .. 59): both called alleles, 53 (slot 0) and 50 (slot 1), in one class.   gene 2 (60 .. 65): slot 1 empty.
    gene 3 (66 .. 69): no call; 66 and 67 weigh the same (groups 10 and 11).   gene 4 (70 .. 72): in no group."""
    q = [900, 500, 300, 200, 100, 50, 4000, 3000, 70, 0, 640, 640, 10]
    holds = {a: {0, 1, 2} for a in range(5, 45)}
    holds.update({0: {0, 3}, 1: {0, 3}, 45: {0, 3, 9}, 46: {5}, 47: {5}, 2: {1, 4}, 3: {4}, 4: {2, 3, 4}, 49: {9}})
    holds.update({50: {6, 7}, 53: {6, 7}, 51: {6}, 52: {7, 8}, 54: {8}, 55: {6, 7, 8}})
    holds.update({60: {0, 6}, 61: {1, 6, 12}, 62: {12}, 63: {0, 1}})
    holds.update({66: {10}, 67: {11}, 68: {10, 11}, 69: {2, 10}})
    gene = [0] * 50 + [1] * 10 + [2] * 6 + [3] * 4 + [4] * 3
    called = [17, 3, 53, 50, 61, -1, -1, -1, -1, -1]
    return HostCase(holds, q, gene, called)


def host_random(seed, n_genes=3, per=8, n_groups=14):
    rng = np.random.default_rng(seed)
    A = n_genes * per
    gene = [a // per for a in range(A)]
    patterns = [frozenset(rng.choice(n_groups, size=int(rng.integers(1, 4)), replace=False).tolist()) for _ in range(6)]   # few patterns: classes form
    holds = {a: set(patterns[int(rng.integers(0, len(patterns)))]) for a in range(A) if rng.random() < 0.9}
    for g in range(n_groups):
        if not any(g in s for s in holds.values()):
            holds.setdefault(int(rng.integers(0, A)), set()).add(g)
    q = rng.integers(0, 5, size=n_groups) * rng.integers(1, 1 << 20, size=n_groups)   # a fifth of the groups weigh nothing
    called = []
    for x in range(n_genes):
        k = int(rng.integers(0, 3))
        mine = rng.permutation(np.arange(x * per, (x + 1) * per)).tolist()
        called += [mine[0] if k >= 1 else -1, mine[1] if k == 2 else -1]
    return HostCase(holds, q.tolist(), gene, called)
