"""Sequential restatement of the per-barcode allele EM in numpy, and the random group tables the tests
feed it.

Every sum the specification orders is formed by np.bincount, which adds its weights one at a time in index order starting from 0.0:
entries are laid out group by group (groups in the barcode's order, each list in ascending allele order), so per group the psum terms
arrive in ascending allele order, per allele the n and f terms in group order, and per barcode the |theta' - theta| terms in ascending
allele order.  Barcodes that have stopped are dropped from the working set, so the cost per update follows the barcodes still running."""
import numpy as np


class Table:
    """Barcodes' group tables in the C ABI's layout (all offsets start at 0)."""

    def __init__(self, bc_allele_ptr, bc_allele, bc_group_ptr, group_count, group_entry_ptr, entry_local):
        self.bc_allele_ptr = np.asarray(bc_allele_ptr, np.uint64)
        self.bc_allele = np.asarray(bc_allele, np.uint32)
        self.bc_group_ptr = np.asarray(bc_group_ptr, np.uint64)
        self.group_count = np.asarray(group_count, np.float64)
        self.group_entry_ptr = np.asarray(group_entry_ptr, np.uint64)
        self.entry_local = np.asarray(entry_local, np.uint32)

    @property
    def n_barcodes(self):
        return len(self.bc_allele_ptr) - 1

    def args(self):
        return (self.bc_allele_ptr, self.bc_allele, self.bc_group_ptr, self.group_count, self.group_entry_ptr, self.entry_local)

    def sizes(self):
        """per barcode: |U_b|, groups, entries"""
        L = np.diff(self.bc_allele_ptr).astype(np.int64)
        G = np.diff(self.bc_group_ptr).astype(np.int64)
        E = self.group_entry_ptr[self.bc_group_ptr.astype(np.int64)].astype(np.int64)
        return L, G, np.diff(E)


def lds_words(L, G, E):
    """the per-wave LDS arena a barcode needs (include/t1k_gpu.h): above the budget it takes the global-memory shape"""
    return 4 * L + 4 * G + (G + 1) + (L + 1) + 2 * E


def from_lists(barcodes):
    """barcodes: per barcode a list of (sorted allele-id tuple, count) in group order -> Table (U_b = union of the lists)"""
    ap, al, gp, gc, ep, el = [0], [], [0], [], [0], []
    for groups in barcodes:
        U = sorted(set(a for s, _ in groups for a in s))
        loc = {a: i for i, a in enumerate(U)}
        al += U
        ap.append(len(al))
        for s, c in groups:
            el += [loc[a] for a in s]
            ep.append(len(el))
            gc.append(float(c))
        gp.append(len(gc))
    return Table(ap, al, gp, gc, ep, el)


def restate(t, rho=None, alpha=0.0, tol=1e-7, max_iter=1000):
    """-> (n laid out as t.bc_allele, updates per barcode)"""
    nB = t.n_barcodes
    L, G, E = t.sizes()
    nL, nG = len(t.bc_allele), len(t.group_count)
    bc_of_allele = np.repeat(np.arange(nB), L)
    bc_of_group = np.repeat(np.arange(nB), G)
    gsize = np.diff(t.group_entry_ptr).astype(np.int64)
    group_of_entry = np.repeat(np.arange(nG), gsize)
    entry_allele = t.entry_local.astype(np.int64) + t.bc_allele_ptr[:-1].astype(np.int64)[bc_of_group][group_of_entry]  # global local-allele index
    N = np.bincount(bc_of_group, weights=t.group_count, minlength=nB)
    prior = np.zeros(nL) if (alpha == 0 or rho is None) else alpha * np.asarray(rho, np.float64)[t.bc_allele]
    f = np.bincount(entry_allele, weights=(t.group_count / gsize.astype(np.float64))[group_of_entry], minlength=nL)
    with np.errstate(invalid="ignore", divide="ignore"):  # (N_b = 0: those barcodes never run)
        theta = f / N[bc_of_allele]
    n = np.zeros(nL)
    iters = np.zeros(nB, np.int32)
    active = N != 0
    it = 0
    # the working set: the entries, groups and alleles of the barcodes still running
    while it < max_iter and active.any():
        ga = active[bc_of_group]
        aa = active[bc_of_allele]
        ea = ga[group_of_entry]
        g_ids = np.nonzero(ga)[0]
        a_ids = np.nonzero(aa)[0]
        e_grp = group_of_entry[ea]
        e_all = entry_allele[ea]
        psum = np.zeros(nG)
        psum[g_ids] = np.bincount(e_grp, weights=theta[e_all], minlength=nG)[g_ids]
        contrib = t.group_count[e_grp] * (theta[e_all] / psum[e_grp])
        n_new = np.bincount(e_all, weights=contrib, minlength=nL)
        n[a_ids] = n_new[a_ids]
        th_new = (n[a_ids] + prior[a_ids]) / (N[bc_of_allele[a_ids]] + alpha)
        d = np.bincount(bc_of_allele[a_ids], weights=np.abs(th_new - theta[a_ids]), minlength=nB)
        theta[a_ids] = th_new
        it += 1
        iters[active] = it
        active = active & ~(d < tol)
    return n, iters


def random_table(rng, n_barcodes, n_alleles=60, max_list=12, fragments=200000, zipf=1.3, big_share=0.0):
    """random group tables with Zipf barcode sizes; lists of 1..max_list alleles drawn from a few per-barcode favourites (so that
    groups repeat); big_share > 0: barcode 0 holds that share of all fragments"""
    w = 1.0 / np.arange(1, n_barcodes + 1) ** zipf
    sizes = np.maximum(1, np.floor(w / w.sum() * fragments)).astype(np.int64)
    rng.shuffle(sizes)
    if big_share > 0:
        sizes[0] = int(big_share * sizes[1:].sum() / (1 - big_share))
    barcodes = []
    for b in range(n_barcodes):
        pool = rng.choice(n_alleles, size=int(rng.integers(1, 25)), replace=False)
        # fragment lists: a bounded menu of patterns per barcode, drawn with skewed frequencies
        menu = []
        for _ in range(int(min(sizes[b], rng.integers(1, 40 if sizes[b] < 1000 else 400)))):
            k = int(rng.integers(1, min(max_list, len(pool)) + 1))
            menu.append(tuple(sorted(rng.choice(pool, size=k, replace=False).tolist())))
        p = rng.random(len(menu)) ** 3 + 1e-3
        draws = rng.choice(len(menu), size=int(sizes[b]), p=p / p.sum())
        order, counts = [], {}
        for d in draws:           # groups in first-appearance order
            s = menu[d]
            if s not in counts:
                counts[s] = 0
                order.append(s)
            counts[s] += 1
        barcodes.append([(s, counts[s]) for s in order])
    return barcodes
