"""A plain restatement of genotyper --bootstrap: the resampling of the read groups, the SQUAREM loop of
Genotyper::QuantifyAlleleEquivalentClass around em_ref.em_update_ref with its masking rule, the statistics and the text of
<prefix>_bootstrap.tsv.  test_boot_cpu.py and test_gpu_boot.py run the library against it.

Integers are Python integers (the hash works modulo 2^64), every floating-point sum is a chain of Python floats added one after the
other in the order the host code adds them, as in em_ref.py; numpy is used for element-wise operations only."""
import decimal
import math

import numpy as np

import em_ref

M64 = (1 << 64) - 1
GOLD, MUL1, MUL2, REP = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB, 0xD1342543DE82EF95
N_THRESHOLDS = 20
HEADER = "#gene\tseries\tcalled\tabundance\tmean\tsd\tq05\tq50\tq95\ttop1\ttop2\tpass\treplicates\n"
MAX_ITERATIONS, MASK_EVERY = 1000, 10


# ------------------------------------------------------------------------------------------------------------------------------------
# the resampling
# ------------------------------------------------------------------------------------------------------------------------------------
def thresholds(digits=120):
    """T_k = floor(2^64 * e^-1 * sum_{j <= k} 1 / j!) for k = 0 .. 19, and T_20 (the first that is 2^64 - 1: not in the table)"""
    with decimal.localcontext() as c:
        c.prec = digits
        inv_e = 1 / decimal.Decimal(1).exp()
        out, s, f = [], decimal.Decimal(0), decimal.Decimal(1)
        for k in range(N_THRESHOLDS + 1):
            if k:
                f *= k
            s += 1 / f
            out.append(int((decimal.Decimal(1 << 64) * inv_e * s).to_integral_value(rounding=decimal.ROUND_FLOOR)))
    return out[:N_THRESHOLDS], out[N_THRESHOLDS]


T = thresholds()[0]


def mix(z):
    z = (z + GOLD) & M64
    z = ((z ^ (z >> 30)) * MUL1) & M64
    z = ((z ^ (z >> 27)) * MUL2) & M64
    return z ^ (z >> 31)


def u(seed, r, g, i):
    return mix(mix(mix(seed ^ ((r * REP) & M64)) ^ g) ^ i)


def poisson(v):
    """X(u): the number of k with u >= T_k"""
    return sum(1 for t in T if v >= t)


def n_of(c):
    """n_g = max(1, llrint(c_g)); Python's round() rounds halves to even, as llrint does in the default rounding mode"""
    return max(1, round(float(c)))


def draws(seed, r, g, n):
    h = mix(mix(seed ^ ((r * REP) & M64)) ^ g)
    return sum(poisson(mix(h ^ i)) for i in range(n))


def resample(count, B, seed, identity=False):
    """(k [B + 1][G] of Python integers, c' [B + 1][G] float64); replicate 0 is the data"""
    count = np.asarray(count, np.float64)
    ns = [n_of(c) for c in count.tolist()]
    k = [[n if (r == 0 or identity) else draws(seed, r, g, n) for g, n in enumerate(ns)] for r in range(B + 1)]
    c = np.array([[float(count[g]) * float(k[r][g]) / float(ns[g]) for g in range(len(ns))] for r in range(B + 1)], np.float64).reshape(B + 1, len(ns))
    return k, c


def non_empty(c_row):
    """a replicate whose counts sum to 0 gets no EM (the counts are not negative: the sum is 0 where every count is)"""
    return em_ref.chain(np.asarray(c_row, np.float64).tolist()) != 0


# ------------------------------------------------------------------------------------------------------------------------------------
# the EM of a replicate: Genotyper::QuantifyAlleleEquivalentClass (Genotyper.hpp:1142-1328) on its counts
# ------------------------------------------------------------------------------------------------------------------------------------
class Classes:
    """what the EM needs besides the rows: members[e] (alleles, ascending), ec_len[e], and per allele its series and gene"""

    def __init__(self, ec, eff_len, weight, series, gene, filter_frac=0.15):
        self.ec, self.series, self.gene, self.weight = (np.asarray(a).tolist() for a in (ec, series, gene, weight))
        self.A = len(self.ec)
        self.E = max(self.ec) + 1 if self.A else 0
        self.members = [[] for _ in range(self.E)]
        for a, e in enumerate(self.ec):
            if e >= 0:
                self.members[e].append(a)
        assert all(self.members)
        eff = np.asarray(eff_len).tolist()
        self.ec_len = np.array([min(eff[a] for a in m) for m in self.members], np.int32)
        self.n_series = max(self.series) + 1
        self.n_genes = max(self.gene) + 1
        self.filter_frac = filter_frac

    def start(self):
        return np.array([float(sum(self.weight[a] for a in m)) for m in self.members], np.float64)


def abundances(cl, n):
    """SetAlleleAbundance (957-1014): (abundance [A], ecAbundance [A], majorAbund [series], geneMaxMajor [genes]) as lists of floats"""
    ab, ecab = [0.0] * cl.A, [0.0] * cl.A
    n = np.asarray(n, np.float64).tolist()
    for e, m in enumerate(cl.members):
        fpk = 0.0
        fpk += n[e]
        with np.errstate(all="ignore"):
            fpk = float(np.float64(fpk) / np.float64(int(cl.ec_len[e])) * np.float64(1000.0))
            each = float(np.float64(fpk) / np.float64(len(m)))
        for a in m:
            ab[a], ecab[a] = each, fpk
    return (ab, ecab) + series_sums(cl, ab)


def series_sums(cl, ab):
    major, gmax = [0.0] * cl.n_series, [0.0] * cl.n_genes
    for a in range(cl.A):
        major[cl.series[a]] += ab[a]
    for a in range(cl.A):
        if major[cl.series[a]] > gmax[cl.gene[a]]:
            gmax[cl.gene[a]] = major[cl.series[a]]
    return major, gmax


def masked_x0(cl, n):
    """the masking of every 10th round: alleles of a series below filter_frac * 0.5 of the gene's largest series lose their abundance;
    x0[e] = the class abundance of the class's first member"""
    ab, ecab, major, gmax = abundances(cl, n)
    for a in range(cl.A):
        if major[cl.series[a]] < cl.filter_frac * 0.5 * gmax[cl.gene[a]]:
            ecab[a] = 0.0
    return np.array([ecab[m[0]] for m in cl.members], np.float64)


def quantify(rows, count, cl, max_rounds=None):
    """the SQUAREM loop on (row_ptr, ec_idx) with these counts: (ecReadCount of the last update, rounds)"""
    row_ptr, ec_idx = rows
    x0 = cl.start()
    n = np.zeros(cl.E, np.float64)
    t = rounds = 0
    upd = lambda x: em_ref.em_update_ref(row_ptr, ec_idx, count, cl.ec_len, x)
    while t < MAX_ITERATIONS:
        rounds += 1
        x1 = upd(x0)[0]
        x2 = upd(x1)[0]
        with np.errstate(all="ignore"):
            x3 = em_ref.squarem_x3(x0, x1, x2)[0]
        x1, n, _ = upd(x3)
        with np.errstate(all="ignore"):
            moved = em_ref.chain(np.abs(x1 - x0).tolist())
        x0 = x1
        if moved < 1e-5 and t < MAX_ITERATIONS - 2:
            t = MAX_ITERATIONS - 2
        if t > 0 and t % MASK_EVERY == 0:
            x0 = masked_x0(cl, n)
        t += 1
        if max_rounds is not None and rounds >= max_rounds:
            break
    return n, rounds


def bootstrap(rows, count, cl, B, seed, identity=False):
    """(abundance [B + 1][A], rounds [B + 1], valid [B + 1]): what t1k_job_bootstrap_matrix returns"""
    _, c = resample(count, B, seed, identity)
    ab = np.zeros((B + 1, cl.A), np.float64)
    rounds, valid = [0] * (B + 1), [False] * (B + 1)
    for r in range(B + 1):
        if not non_empty(c[r]):
            continue
        n, rounds[r] = quantify(rows, c[r], cl)
        ab[r] = abundances(cl, n)[0]
        valid[r] = bool(np.isfinite(ab[r]).all())
    return ab, rounds, valid


# ------------------------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------------------------
def quantile_index(p, V):
    return max(0, (p * V + 99) // 100 - 1)


def stats_of(values):
    """(mean, sd, q05, q50, q95) of one series over the valid replicates, in replicate order; all 0 without a valid replicate"""
    V = len(values)
    if V == 0:
        return (0.0,) * 5
    mean = em_ref.chain(values) / float(V)
    sd = 0.0
    if V >= 2:
        ss = 0.0
        for x in values:
            d = x - mean
            ss += d * d
        sd = math.sqrt(ss / float(V - 1))
    asc = sorted(values)
    return (mean, sd) + tuple(asc[quantile_index(p, V)] for p in (5, 50, 95))


def table(matrix, valid, series, gene, called, filter_frac=0.15):
    """matrix [B + 1][A], valid [B + 1]; series[a], gene[a]; called: per gene (series of slot 1, series of slot 2), each in its field's
    order.  -> rows (gene, series, called text, abundance, mean, sd, q05, q50, q95, top1, top2, pass, V) in file order"""
    matrix = np.asarray(matrix, np.float64)
    cl = Classes([-1] * len(series), [1] * len(series), [1] * len(series), series, gene, filter_frac) if len(series) else None
    n_series, n_genes = cl.n_series, len(called)
    gene_of = [-1] * n_series
    for a in range(cl.A):
        gene_of[cl.series[a]] = cl.gene[a]
    of_gene = [[m for m in range(n_series) if gene_of[m] == g] for g in range(n_genes)]
    values = [[] for _ in range(n_series)]
    top1, top2, passed = [0] * n_series, [0] * n_series, [0] * n_series
    V = 0
    for r in range(1, matrix.shape[0]):
        if not valid[r]:
            continue
        V += 1
        major, gmax = series_sums(cl, matrix[r].tolist())
        for m in range(n_series):
            values[m].append(major[m])
        for g in range(n_genes):
            ranked = sorted((m for m in of_gene[g] if major[m] > 0), key=lambda m: (-major[m], m))
            for j, m in enumerate(ranked[:2]):
                top2[m] += 1
                top1[m] += j == 0
            for m in of_gene[g]:
                if major[m] > 0 and not major[m] < filter_frac * gmax[g]:
                    passed[m] += 1
    data = series_sums(cl, matrix[0].tolist())[0]
    rows = []
    for g in range(n_genes):
        s1, s2 = called[g]
        lines = list(s1) + [m for m in s2 if m not in s1]
        rest = [m for m in of_gene[g] if m not in lines and top2[m] > 0]
        rest.sort(key=lambda m: (-top2[m], -stats_of(values[m])[0], m))
        for m in lines + rest:
            text = "1,2" if m in s1 and m in s2 else "1" if m in s1 else "2" if m in s2 else "."
            rows.append((g, m, text, data[m]) + stats_of(values[m]) + (top1[m], top2[m], passed[m], V))
    return rows


def text(rows, gene_names, series_names):
    out = HEADER
    for r in rows:
        out += "%s\t%s\t%s\t" % (gene_names[r[0]], series_names[r[1]], r[2]) + "\t".join("%.6f" % v for v in r[3:9]) + "\t%d\t%d\t%d\t%d\n" % r[9:]
    return out
