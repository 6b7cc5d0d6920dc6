"""Restatement of the alternatives table (genotyper --alternatives, t1k_alt_batch) in plain Python over Python integers:
tables() is what the kernel computes, lines() / text() what the genotyper ranks and writes, brute() the same four sums from sets of
groups -- the definition read literally -- for the CPU tests.  Nothing here imports the product."""
import math

EMPTY = 0xFFFFFFFF
UNIT = 1 << 20
HEADER = "#gene\tcalled\tslot\trank\talt\ttotal_called\ttotal_alt\tshared\tlost\tgained\tunexplained\talt_abundance\tidentical\n"


def q_of(count):
    """the fixed-point weight of a group whose EM count is `count`: llrint(count * 2^20) (round half to even, as the default rounding mode)"""
    x = float(count) * UNIT
    assert x == x and 0 <= x < 2.0 ** 63
    f = math.floor(x)
    d = x - f
    if d > 0.5 or (d == 0.5 and f % 2 == 1):
        f += 1
    return int(f)


def tables(group_ptr, alleles, q, allele_gene, slot_of):
    """[total, both0, both1, neither], each a list of Python ints over the alleles"""
    A = len(allele_gene)
    total, both0, both1, neither = [0] * A, [0] * A, [0] * A, [0] * A
    for g in range(len(group_ptr) - 1):
        row = [int(a) for a in alleles[int(group_ptr[g]):int(group_ptr[g + 1])]]
        present = set(int(slot_of[a]) for a in row if int(slot_of[a]) != EMPTY)
        w = int(q[g])
        for a in row:
            gene = int(allele_gene[a])
            total[a] += w
            if 2 * gene in present:
                both0[a] += w
            if 2 * gene + 1 in present:
                both1[a] += w
            if 2 * gene not in present and 2 * gene + 1 not in present:
                neither[a] += w
    return [total, both0, both1, neither]


def brute(group_ptr, alleles, q, allele_gene, slot_of):
    """the same sums from the definition: per allele the set of groups that hold it, and set algebra with the called alleles' sets"""
    A = len(allele_gene)
    holds = [set() for _ in range(A)]
    for g in range(len(group_ptr) - 1):
        for a in alleles[int(group_ptr[g]):int(group_ptr[g + 1])]:
            holds[int(a)].add(g)
    called = {int(s): a for a, s in enumerate(slot_of) if int(s) != EMPTY}
    weight = lambda groups: sum(int(q[g]) for g in groups)
    out = [[0] * A for _ in range(4)]
    for b in range(A):
        gene = int(allele_gene[b])
        s0 = holds[called[2 * gene]] if 2 * gene in called else set()
        s1 = holds[called[2 * gene + 1]] if 2 * gene + 1 in called else set()
        out[0][b] = weight(holds[b])
        out[1][b] = weight(holds[b] & s0)
        out[2][b] = weight(holds[b] & s1)
        out[3][b] = weight(holds[b] - s0 - s1)
    return out


def lines(tabs, allele_gene, slot_of, top):
    """one tuple per line of the file, in its order: (gene, called allele, slot, rank, alt allele or None, total_called, total_alt, shared,
    lost, gained, unexplained, identical).  Genes ascending, slot 0 before slot 1."""
    total, both, neither = tabs[0], (tabs[1], tabs[2]), tabs[3]
    out = []
    for s, slot in sorted(((a, int(v)) for a, v in enumerate(slot_of) if int(v) != EMPTY), key=lambda x: x[1]):
        gene, k = slot >> 1, slot & 1
        assert int(allele_gene[s]) == gene
        alts, identical = [], 0
        for b in range(len(allele_gene)):
            if b == s or int(allele_gene[b]) != gene or total[b] == 0:
                continue
            shared = both[k][b]
            lost, gained = total[s] - shared, total[b] - shared
            assert lost >= 0 and gained >= 0
            if lost == 0 and gained == 0:
                identical += 1
                continue
            alts.append((lost, -gained, b))
        alts.sort()
        if not alts:
            out.append((gene, s, k, 0, None, total[s], 0, 0, 0, 0, 0, identical))
        for i, (lost, neg, b) in enumerate(alts[:top]):
            out.append((gene, s, k, i + 1, b, total[s], total[b], both[k][b], lost, -neg, neither[b], identical))
    return out


def fmt(v):
    return "%.3f" % (v / float(UNIT))


def text(tabs, allele_gene, slot_of, top, gene_names, allele_names, abundance):
    """the file, byte for byte; abundance[b] a float (printed with %f, as _genotype.tsv prints abundances)"""
    out = [HEADER]
    for gene, s, k, rank, b, tc, ta, sh, lost, gained, un, ident in lines(tabs, allele_gene, slot_of, top):
        out.append("\t".join([gene_names[gene], allele_names[s], str(k), str(rank), "." if b is None else allele_names[b], fmt(tc), fmt(ta), fmt(sh), fmt(lost), fmt(gained),
                              fmt(un), "%f" % (0.0 if b is None else abundance[b]), str(ident)]) + "\n")
    return "".join(out)
