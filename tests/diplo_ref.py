"""Restatement of the diplotype table (genotyper --diplotypes, t1k_diplo_batch) in plain Python over Python integers and
frozensets: plan() forms the classes, the candidates and the groups over candidate ids as the genotyper does, matrix() is what the kernel
computes, lines() / text() what the genotyper ranks and writes, brute() the same quantities from sets of group indices -- the definition
read literally -- for the CPU tests.  Nothing here imports the product."""
from alt_ref import UNIT, fmt, q_of  # noqa: F401  (the weights are those of §14)

HEADER = "#gene\trank\tallele1\tallele2\texplained\tonly1\tonly2\tshared\tunexplained\tequiv1\tequiv2\tcalled\tn_cand\tn_class\n"


class Plan:
    """cand_ptr [genes + 1]; per candidate: rep (the allele that names its class), equiv (class size - 1), total; per gene: n_class, weight
    (W); called_cand [2 * genes] (-1: empty slot); the groups of weight > 0 that hold a candidate, over candidate ids: group_ptr, ent, q"""


def _rows(group_ptr, alleles):
    return [[int(a) for a in alleles[int(group_ptr[g]):int(group_ptr[g + 1])]] for g in range(len(group_ptr) - 1)]


def _choose(classes, max_cand):
    """classes: (total, rep, size, is_called) sorted by total descending, rep ascending -> the candidates, in that order"""
    keep = list(classes[:max_cand])
    for c in classes[max_cand:]:
        if not c[3]:
            continue
        last = max(k for k, d in enumerate(keep) if not d[3])   # the last one that is not called is displaced
        del keep[last]
        keep.append(c)
    keep.sort(key=lambda c: (-c[0], c[1]))
    return keep


def plan(group_ptr, alleles, q, allele_gene, called, max_cand):
    """called[2 * gene + k]: the allele called in slot k of the gene, -1 for none"""
    rows = _rows(group_ptr, alleles)
    A, n_genes = len(allele_gene), len(called) // 2
    member = [set() for _ in range(A)]
    weight = [0] * n_genes
    for g, row in enumerate(rows):
        if int(q[g]) == 0:
            continue
        for a in row:
            member[a].add(g)
        for x in set(int(allele_gene[a]) for a in row):
            weight[x] += int(q[g])
    member = [frozenset(m) for m in member]
    total = [sum(int(q[g]) for g in m) for m in member]
    p = Plan()
    p.cand_ptr, p.rep, p.equiv, p.total, p.n_class, p.weight, p.called_cand = [0], [], [], [], [], weight, [-1] * (2 * n_genes)
    cand_of = {}
    for x in range(n_genes):
        by_set = {}
        for a in range(A):
            if int(allele_gene[a]) == x and total[a] > 0:
                by_set.setdefault(member[a], []).append(a)
        classes = []
        for m, mine in by_set.items():
            rep = min(mine)
            is_called = False
            for k in (1, 0):                                    # slot 0 before slot 1
                if int(called[2 * x + k]) in mine:
                    rep, is_called = int(called[2 * x + k]), True
            classes.append((total[rep], rep, len(mine), is_called, m))
        classes.sort(key=lambda c: (-c[0], c[1]))
        p.n_class.append(len(classes))
        for t, rep, size, _, m in _choose(classes, max_cand):
            cand_of[rep] = len(p.rep)
            for k in (0, 1):
                s = int(called[2 * x + k])
                if s >= 0 and total[s] > 0 and member[s] == m:
                    p.called_cand[2 * x + k] = len(p.rep)
            p.rep.append(rep)
            p.equiv.append(size - 1)
            p.total.append(t)
        p.cand_ptr.append(len(p.rep))
    p.group_ptr, p.ent, p.q = [0], [], []
    for g, row in enumerate(rows):
        ids = sorted(cand_of[a] for a in row if a in cand_of)
        if int(q[g]) == 0 or not ids:
            continue
        p.ent += ids
        p.group_ptr.append(len(p.ent))
        p.q.append(int(q[g]))
    return p


def matrix(group_ptr, ent, q, cand_ptr):
    """the output of t1k_diplo_batch as a flat list of Python ints: per gene its n * n block, cell (i, j) at i * n + j, i <= j"""
    n_genes = len(cand_ptr) - 1
    base, gene_of = [0], []
    for x in range(n_genes):
        n = int(cand_ptr[x + 1]) - int(cand_ptr[x])
        base.append(base[-1] + n * n)
        gene_of += [x] * n
    out = [0] * base[-1]
    for g, row in enumerate(_rows(group_ptr, ent)):
        w = int(q[g])
        for u, i in enumerate(row):
            x = gene_of[i]
            lo, n = int(cand_ptr[x]), int(cand_ptr[x + 1]) - int(cand_ptr[x])
            for j in row[u:]:
                if j >= lo + n:
                    break
                out[base[x] + (i - lo) * n + (j - lo)] += w
    return out


def brute(group_ptr, alleles, q, allele_gene, called, max_cand):
    """per gene: ([(rep, equiv, total) of every candidate, in order], n_class, W, {(i, j): M}) from the sets of groups that hold each allele"""
    rows = _rows(group_ptr, alleles)
    A, n_genes = len(allele_gene), len(called) // 2
    holds = [frozenset(g for g, row in enumerate(rows) if a in row and int(q[g]) > 0) for a in range(A)]
    w = lambda groups: sum(int(q[g]) for g in groups)
    out = []
    for x in range(n_genes):
        mine = [a for a in range(A) if int(allele_gene[a]) == x]
        classes = []
        for s in set(holds[a] for a in mine if w(holds[a]) > 0):
            same = [a for a in mine if holds[a] == s]
            named = [int(called[2 * x + k]) for k in (0, 1) if int(called[2 * x + k]) in same]
            classes.append((w(s), named[0] if named else same[0], len(same), bool(named)))
        classes.sort(key=lambda c: (-c[0], c[1]))
        cand = _choose(classes, max_cand)
        M = {(i, j): w(holds[cand[i][1]] & holds[cand[j][1]]) for i in range(len(cand)) for j in range(i, len(cand))}
        union = frozenset().union(*[holds[a] for a in mine]) if mine else frozenset()
        out.append(([(c[1], c[2] - 1, c[0]) for c in cand], len(classes), w(union), M))
    return out


def lines(p, mat, top):
    """one tuple per line of the file, in its order: (gene, rank, allele1, allele2, explained, only1, only2, shared, unexplained, equiv1,
    equiv2, called, n_cand, n_class); allele1 / allele2 are the alleles that name the classes"""
    out, base = [], 0
    for x in range(len(p.cand_ptr) - 1):
        lo, n = p.cand_ptr[x], p.cand_ptr[x + 1] - p.cand_ptr[x]
        M = lambda i, j: int(mat[base + i * n + j])
        pairs = []
        for i in range(n):
            for j in range(i, n):
                sh = M(i, j)
                o1, o2 = M(i, i) - sh, M(j, j) - sh
                assert o1 >= 0 and o2 >= 0 and (i != j or o1 == o2 == 0)
                pairs.append((-(M(i, i) + M(j, j) - sh), -min(o1, o2), i, j))
        pairs.sort()
        ci, cj = p.called_cand[2 * x], p.called_cand[2 * x + 1]
        ci = cj if ci < 0 else ci
        cj = ci if cj < 0 else cj
        want = (min(ci, cj) - lo, max(ci, cj) - lo) if ci >= 0 else None
        for r, (ne, _, i, j) in enumerate(pairs):
            if r < top or (i, j) == want:
                sh = M(i, j)
                out.append((x, r + 1, p.rep[lo + i], p.rep[lo + j], -ne, M(i, i) - sh, M(j, j) - sh, sh, p.weight[x] + ne, p.equiv[lo + i], p.equiv[lo + j],
                            1 if (i, j) == want else 0, n, p.n_class[x]))
        base += n * n
    return out


def text(p, mat, top, gene_names, allele_names):
    """the file, byte for byte"""
    out = [HEADER]
    for x, rank, a1, a2, ex, o1, o2, sh, un, e1, e2, called, n_cand, n_class in lines(p, mat, top):
        out.append("\t".join([gene_names[x], str(rank), allele_names[a1], allele_names[a2], fmt(ex), fmt(o1), fmt(o2), fmt(sh), fmt(un), str(e1), str(e2), str(called),
                              str(n_cand), str(n_class)]) + "\n")
    return "".join(out)
