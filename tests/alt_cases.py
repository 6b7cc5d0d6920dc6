"""Inputs of the alternatives tests (t1k_alt_batch): a designed table of read groups that holds every case the kernel can go
wrong at, random small tables, and the inputs the C ABI must refuse.  Shared by test_alt_cpu.py and test_gpu_alt.py."""
import numpy as np

EMPTY = 0xFFFFFFFF
SIZES = (1, 2, 63, 64, 65, 128, 129, 257)


class Case:
    def __init__(self, groups, q, allele_gene, slot_of, n_genes):
        self.groups = [sorted(int(a) for a in g) for g in groups]
        self.group_ptr = np.concatenate([[0], np.cumsum([len(g) for g in self.groups])]).astype(np.uint64)
        self.alleles = np.array([a for g in self.groups for a in g], dtype=np.uint32)
        self.q = np.array(q, dtype=np.uint64)
        self.allele_gene = np.array(allele_gene, dtype=np.uint32)
        self.slot_of = np.array(slot_of, dtype=np.uint32)
        self.n_genes = n_genes
        assert len(self.q) == len(self.groups) and len(self.allele_gene) == len(self.slot_of)
        for a in (self.group_ptr, self.alleles, self.q, self.allele_gene, self.slot_of):
            a.setflags(write=False)

    def args(self):
        return self.group_ptr, self.alleles, self.q, self.allele_gene, self.slot_of


def designed(seed=5):
    """5 genes of 80 alleles each, allele a in gene a % 5, so that a group of ascending alleles runs through the genes.  Calls:
    gene 0: alleles 0 (slot 0) and 395 (slot 1) -- the first and the last entry of every group that holds them;
    gene 1: allele 201 in slot 0, slot 1 empty;  gene 2: 102 (slot 0) and 297 (slot 1);  gene 3: no call;  gene 4: 4 (slot 0) and 399
    (slot 1), the last allele of all.
    Groups: for every size in SIZES, one group per pattern of called alleles -- none, only slot 0 of gene 0, only slot 1 of gene 0, both,
    calls of two genes with different patterns, calls of three genes with different patterns, the called allele first, the called allele
    last -- filled up with alleles that are not called."""
    rng = np.random.default_rng(seed)
    n_genes, per = 5, 80
    A = n_genes * per
    allele_gene = [a % n_genes for a in range(A)]
    slot_of = [EMPTY] * A
    calls = {0: 0, 1: 395, 2: 201, 4: 102, 5: 297, 8: 4, 9: 399}
    for slot, a in calls.items():
        assert allele_gene[a] == slot >> 1
        slot_of[a] = slot
    plain = [a for a in range(A) if slot_of[a] == EMPTY]
    patterns = {
        "none": [],
        "slot0": [0],
        "slot1": [395],
        "both": [0, 395],
        "two_genes": [0, 297],            # gene 0: slot 0 only, gene 2: slot 1 only
        "three_genes": [0, 395, 201, 102],  # gene 0: both, gene 1: its only slot, gene 2: slot 0 only (genes 3 and 4: nothing)
        "first": [0],
        "last": [399],
    }
    groups, q, tags = [], [], []
    for n in SIZES:
        for name, must in patterns.items():
            must = must[:n]
            fill = rng.choice(plain, size=n - len(must), replace=False).tolist()
            groups.append(must + fill)
            q.append(int(rng.integers(1, 1 << 22)))
            tags.append((n, name))
    # a few weights of another magnitude, and two groups that hold the same alleles (coalescing never produces them; the sums do not care)
    q[3] = (1 << 40) + 12345
    q[17] = 1
    groups.append(list(groups[11]))
    q.append(777)
    tags.append((len(groups[11]), "twin"))
    c = Case(groups, q, allele_gene, slot_of, n_genes)
    c.tags = tags
    return c


def random_case(seed, n_genes=4, per=6, n_groups=40, max_size=10):
    rng = np.random.default_rng(seed)
    A = n_genes * per
    allele_gene = rng.integers(0, n_genes, size=A).tolist()
    slot_of = [EMPTY] * A
    for g in range(n_genes):
        mine = [a for a in range(A) if allele_gene[a] == g]
        rng.shuffle(mine)
        k = int(rng.integers(0, 3))      # no call, one call, two calls
        for slot, a in zip((2 * g, 2 * g + 1)[:k], mine):
            slot_of[a] = slot
    groups = [rng.choice(A, size=int(rng.integers(1, min(max_size, A) + 1)), replace=False).tolist() for _ in range(n_groups)]
    q = rng.integers(1, 1 << 24, size=n_groups).tolist()
    return Case(groups, q, allele_gene, slot_of, n_genes)


def word_edge_case(n_genes, seed=9):
    """two alleles called in each of the last two genes (slots 2 * n_genes - 4 .. 2 * n_genes - 1) and in gene 0; three alleles per gene"""
    rng = np.random.default_rng(seed + n_genes)
    A = 3 * n_genes
    allele_gene = [a // 3 for a in range(A)]
    slot_of = [EMPTY] * A
    for g in (0, n_genes - 2, n_genes - 1):
        slot_of[3 * g] = 2 * g
        slot_of[3 * g + 2] = 2 * g + 1
    groups = []
    for n in (1, 3, 30, 70, min(A, 200)):
        for _ in range(6):
            groups.append(rng.choice(A, size=min(n, A), replace=False).tolist())
    tail = list(range(A - 6, A))
    groups += [tail, tail[:3], tail[3:], [A - 1], [A - 3], [A - 4, A - 1], [0, A - 1]]
    q = rng.integers(1, 1 << 30, size=len(groups)).tolist()
    return Case(groups, q, allele_gene, slot_of, n_genes)


def refusals():
    """name -> (expected code name, argument tuple (group_ptr, alleles, q, allele_gene, n_genes, slot_of)); the sound input they are all
    one change away from is the first entry, 'sound'"""
    gp = np.array([0, 3, 5], dtype=np.uint64)
    al = np.array([0, 2, 3, 1, 2], dtype=np.uint32)
    q = np.array([5, 7], dtype=np.uint64)
    gene = np.array([0, 0, 1, 1], dtype=np.uint32)
    slot = np.array([0, 1, 2, EMPTY], dtype=np.uint32)

    def edit(a, i, v):
        b = a.copy()
        b[i] = v
        return b
    return {
        "sound": ("OK", (gp, al, q, gene, 2, slot)),
        "ptr_start": ("ARG", (edit(gp, 0, 1), al, q, gene, 2, slot)),
        "ptr_decreases": ("ARG", (np.array([0, 5, 3], dtype=np.uint64), al, q, gene, 2, slot)),
        "allele_range": ("ARG", (gp, edit(al, 4, 4), q, gene, 2, slot)),
        "duplicate": ("ARG", (gp, edit(al, 1, 0), q, gene, 2, slot)),
        "descending": ("ARG", (gp, edit(al, 3, 3), q, gene, 2, slot)),
        "gene_range": ("ARG", (gp, al, q, edit(gene, 3, 2), 2, slot)),
        "slot_of_other_gene": ("ARG", (gp, al, q, gene, 2, edit(slot, 3, 1))),
        "slot_out_of_range": ("ARG", (gp, al, q, gene, 2, edit(slot, 3, 4))),
        "slot_claimed_twice": ("ARG", (gp, al, q, gene, 2, edit(slot, 3, 2))),
        "sum_2_63": ("CAPACITY", (gp, al, np.array([1 << 62, 1 << 62], dtype=np.uint64), gene, 2, slot)),
        "q_2_63": ("CAPACITY", (gp, al, np.array([1 << 63, 0], dtype=np.uint64), gene, 2, slot)),
    }
