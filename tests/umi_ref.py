"""The UMI collapse of DESIGN §11.2 (t1k_umi_collapse, analyzer --umi) restated in plain Python / numpy, and the generated table the
tests run it on.  Nothing here imports the package: the GPU tests compare the kernels against restate() exactly, frac bit for bit."""
import numpy as np

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
BASES = "ACGT"


def encode(umi):
    """UMI text -> word: code in bits 0-31 (first base most significant), length in bits 32-36; NONE if it is not 1-16 of ACGT"""
    if not 1 <= len(umi) <= 16 or any(c not in BASES for c in umi):
        return NONE
    code = 0
    for c in umi:
        code = code * 4 + BASES.index(c)
    return np.uint64(code | (len(umi) << 32))


def decode(word):
    word = int(word)
    n, code = word >> 32, word & 0xFFFFFFFF
    return "".join(BASES[(code >> (2 * (n - 1 - i))) & 3] for i in range(n))


class Table:
    """fragments: row, UMI word, ascending allele list (CSR); allele -> gene"""

    def __init__(self, frag_row, frag_umi, list_ptr, list_allele, n_rows, allele_gene, n_genes):
        self.frag_row = np.ascontiguousarray(frag_row, np.uint32)
        self.frag_umi = np.ascontiguousarray(frag_umi, np.uint64)
        self.list_ptr = np.ascontiguousarray(list_ptr, np.uint64)
        self.list_allele = np.ascontiguousarray(list_allele, np.uint32)
        self.n_rows = int(n_rows)
        self.allele_gene = np.ascontiguousarray(allele_gene, np.uint32)
        self.n_genes = int(n_genes)

    @property
    def n_alleles(self):
        return len(self.allele_gene)

    @property
    def n_frag(self):
        return len(self.frag_row)

    def lists(self):
        lp = self.list_ptr.astype(np.int64)
        return [tuple(int(a) for a in self.list_allele[lp[f]:lp[f + 1]]) for f in range(self.n_frag)]

    def args(self):
        return (self.frag_row, self.frag_umi, self.list_ptr, self.list_allele, self.n_rows, self.allele_gene, self.n_genes)


def from_fragments(frags, n_rows, allele_gene, n_genes):
    """frags: (row, UMI text or None, iterable of alleles)"""
    row, umi, ptr, al = [], [], [0], []
    for r, u, l in frags:
        row.append(r)
        umi.append(NONE if u is None else encode(u))
        al.extend(sorted(set(l)))
        ptr.append(len(al))
    return Table(row, np.array(umi, np.uint64), ptr, al, n_rows, allele_gene, n_genes)


class Result:
    pass


def _parents(keys, counts, mismatch):
    """keys: the distinct (bucket << 32 | code) ascending, counts beside them -> parent index of each (itself: none)"""
    n = len(keys)
    parent = np.arange(n, dtype=np.int64)
    if not mismatch or n == 0:
        return parent
    length = ((keys >> np.uint64(32)) & np.uint64(15)).astype(np.int64) + 1
    code = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    best_cnt = np.zeros(n, np.int64)
    best_code = np.zeros(n, np.int64)
    for p in range(16):
        live = length > p
        if not live.any():
            break
        for x in (1, 2, 3):
            want = keys ^ np.uint64(x << (2 * p))
            at = np.searchsorted(keys, want)
            at_c = np.minimum(at, n - 1)
            found = live & (at < n) & (keys[at_c] == want)
            cv = counts[at_c]
            v = code ^ (x << (2 * p))
            cand = found & (cv >= 2 * counts - 1) & ((cv > counts) | ((cv == counts) & (v < code)))
            better = cand & ((cv > best_cnt) | ((cv == best_cnt) & (v < best_code)))
            parent[better] = at_c[better]
            best_cnt[better] = cv[better]
            best_code[better] = v[better]
    return parent


def restate(t, mismatch=1):
    """-> Result: frag_mol, mol_row, mol_frags, mol_lists (canonical order: row, then smallest fragment), frac, uniq [n_rows, n_alleles],
    stats, and what the coverage test looks at (parent of every distinct UMI, hops, ties, buckets, split keys, cross-gene lists)"""
    F, A = t.n_frag, t.n_alleles
    lists = t.lists()
    has = t.frag_umi != NONE
    first = t.list_allele[t.list_ptr[:-1].astype(np.int64)] if F else np.zeros(0, np.uint32)
    gene = t.allele_gene[first].astype(np.uint64)
    length = (t.frag_umi >> np.uint64(32)) & np.uint64(31)
    bucket = ((t.frag_row.astype(np.uint64) * np.uint64(t.n_genes) + gene) << np.uint64(4)) | (length - np.uint64(1))
    key = (bucket << np.uint64(32)) | (t.frag_umi & np.uint64(0xFFFFFFFF))
    keys, inv, counts = np.unique(key[has], return_inverse=True, return_counts=True)
    counts = counts.astype(np.int64)
    parent = _parents(keys, counts, mismatch)
    root = parent.copy()
    hops = (parent != np.arange(len(keys))).astype(np.int64)
    while True:
        nxt = parent[root]
        moved = nxt != root
        if not moved.any():
            break
        hops += moved
        root = nxt
    # keys: (bucket, root) -> their fragments; a fragment without a UMI is a key of its own
    frag_key = np.empty(F, np.int64)
    frag_key[has] = root[inv]
    frag_key[~has] = len(keys) + np.arange(int((~has).sum()))
    order = np.argsort(frag_key, kind="stable")
    cuts = np.flatnonzero(np.diff(frag_key[order])) + 1
    mols = []  # (row, fragments, list)
    split = 0
    for grp in np.split(order, cuts):
        grp = [int(f) for f in grp]
        common = set(lists[grp[0]])
        for f in grp[1:]:
            common &= set(lists[f])
        if common:
            mols.append((int(t.frag_row[grp[0]]), grp, tuple(sorted(common))))
            continue
        split += 1
        by_list = {}
        for f in grp:
            by_list.setdefault(lists[f], []).append(f)
        for l, fs in by_list.items():
            mols.append((int(t.frag_row[fs[0]]), fs, l))
    mols.sort(key=lambda m: (m[0], min(m[1])))
    r = Result()
    r.frag_mol = np.zeros(F, np.uint32)
    for i, (_, fs, _) in enumerate(mols):
        r.frag_mol[fs] = i
    r.mol_row = np.array([m[0] for m in mols], np.uint32)
    r.mol_frags = np.array([len(m[1]) for m in mols], np.uint32)
    r.mol_lists = [m[2] for m in mols]
    max_n = max([len(l) for l in r.mol_lists] + [1])
    K = np.zeros((t.n_rows * A, max_n + 1), np.int64)
    for row, _, l in mols:
        for a in l:
            K[row * A + a, len(l)] += 1
    frac = np.zeros(t.n_rows * A, np.float64)
    for n in range(1, max_n + 1):
        frac = frac + K[:, n].astype(np.float64) / np.float64(n)
    r.frac = frac.reshape(t.n_rows, A)
    r.uniq = K[:, 1].astype(np.int32).reshape(t.n_rows, A)
    n_keys = len(np.unique(root))
    r.stats = dict(distinct=len(keys), keys=n_keys, corrected=int((parent != np.arange(len(keys))).sum()), split=split, no_umi=int((~has).sum()))
    r.keys, r.counts, r.parent, r.hops = keys, counts, parent, hops
    r.ties = int((counts[parent] == counts)[parent != np.arange(len(keys))].sum())
    r.buckets = len(np.unique(keys >> np.uint64(32)))
    r.max_bucket_fragments = int(np.bincount(np.unique(bucket[has], return_inverse=True)[1]).max()) if has.any() else 0
    r.cross_gene = int(sum(1 for l in lists if len({int(t.allele_gene[a]) for a in l}) > 1))
    r.lengths = sorted({int(x) for x in length[has]})
    return r


def even_split(t):
    """the fragment table: every fragment's list counted 1 / n per allele (what _barcode_expr.tsv holds)"""
    A = t.n_alleles
    frac = np.zeros((t.n_rows, A))
    uniq = np.zeros((t.n_rows, A), np.int32)
    for f, l in enumerate(t.lists()):
        for a in l:
            frac[t.frag_row[f], a] += 1.0 / len(l)
            if len(l) == 1:
                uniq[t.frag_row[f], a] += 1
    return frac, uniq


def distinct_umis(n, length=12):
    """n UMI texts at pairwise Hamming distance >= 2: the index in base 4 and a check base (the sum of the digits mod 4)"""
    assert n <= 4 ** (length - 1)
    out = []
    for i in range(n):
        d = [(i >> (2 * j)) & 3 for j in range(length - 1)]
        out.append("".join(BASES[x] for x in d) + BASES[sum(d) & 3])
    return out


def generate(seed=11, fragments=200000, rows=2000, genes=6, per_gene=10):
    """the table of the GPU test: Zipf row sizes with one row holding 30 % of the fragments; lists of 1-6 alleles of one gene, 5 % with
    an extra allele of any gene; UMI length 8 / 12 / 10 by row; UMIs from a per-row pool a third of the row's size with repeated 20 %
    single-base mutations; 1 % of the fragments without a UMI"""
    rng = np.random.default_rng(seed)
    A = genes * per_gene
    allele_gene = np.repeat(np.arange(genes), per_gene).astype(np.uint32)
    big = int(0.3 * fragments)
    w = 1.0 / np.arange(1, rows)
    rest = rng.choice(np.arange(1, rows), size=fragments - big, p=w / w.sum())
    frag_row = np.concatenate([np.zeros(big, np.int64), rest])
    rng.shuffle(frag_row)
    # lists
    g = rng.integers(0, genes, fragments)
    k = rng.integers(1, 7, fragments)
    extra = rng.random(fragments) < 0.05
    extra_al = rng.integers(0, A, fragments)
    ptr, al = [0], []
    for f in range(fragments):
        l = set((g[f] * per_gene + rng.choice(per_gene, k[f], replace=False)).tolist())
        if extra[f]:
            l.add(int(extra_al[f]))
        al.extend(sorted(l))
        ptr.append(len(al))
    # UMIs
    length = np.array([8, 12, 10])[frag_row % 3]
    code = np.zeros(fragments, np.int64)
    size = np.bincount(frag_row, minlength=rows)
    for r in range(rows):
        if not size[r]:
            continue
        L = (8, 12, 10)[r % 3]
        pool = rng.integers(0, 4 ** L, max(1, size[r] // 3))
        code[frag_row == r] = pool[rng.integers(0, len(pool), size[r])]
    live = np.ones(fragments, bool)
    while live.any():
        live &= rng.random(fragments) < 0.2
        pos = (rng.random(fragments) * length).astype(np.int64)
        x = rng.integers(1, 4, fragments)
        code[live] ^= (x << (2 * pos))[live]
    umi = (code | (length << 32)).astype(np.uint64)
    umi[rng.random(fragments) < 0.01] = NONE
    return Table(frag_row, umi, ptr, al, rows, allele_gene, genes)
