"""Restatement of the two stages of t1k_dedupe.hip in plain Python: no packing, no hashing, strings and dictionaries only.

collapse()  what t1k_reads_dedupe computes inside one window (Genotyper.cpp:451-480 sorts the read-ends and assigns every distinct one once,
            with its multiplicity as the weight);
link()      what t1k_xwin_link / t1k_xwin_resolve compute across the windows of a job: which distinct read-ends of a window an earlier
            window holds already, and where.

Two read-ends are the same exactly when their strings are equal after every character outside ACGT has become N (README, "Limits")."""


def canonical(read):
    """the read as the stages see it: every character outside A C G T is N (lower case included)"""
    return "".join(c if c in "ACGT" else "N" for c in read)


def collapse(reads, weights=None):
    """(distinct_of, representatives, weight_of_distinct): distinct_of[i] = number of read i's sequence, the sequences numbered in the order
    of their first use; representatives[d] = the first read with sequence d; weight_of_distinct[d] = the sum of the weights of the reads
    with sequence d (1 each when no weights are given)"""
    number = {}
    distinct_of, representatives, weight_of_distinct = [], [], []
    for i, read in enumerate(reads):
        key = canonical(read)
        if key not in number:
            number[key] = len(representatives)
            representatives.append(i)
            weight_of_distinct.append(0)
        d = number[key]
        distinct_of.append(d)
        weight_of_distinct[d] += 1 if weights is None else int(weights[i])
    return distinct_of, representatives, weight_of_distinct


def collapse_neighbours(reads, weights=None):
    """collapse() for a build whose hashes all collide (T1K_TEST_DEDUPE_HASH_BITS=0): t1k_reads_dedupe splits a run of equal hashes wherever
    two neighbours in upload order differ, so only neighbours merge -- a collision costs a merge, never makes one"""
    distinct_of, representatives, weight_of_distinct = [], [], []
    for i, read in enumerate(reads):
        if i == 0 or canonical(read) != canonical(reads[i - 1]):
            representatives.append(i)
            weight_of_distinct.append(0)
        distinct_of.append(len(representatives) - 1)
        weight_of_distinct[-1] += 1 if weights is None else int(weights[i])
    return distinct_of, representatives, weight_of_distinct


def link(windows):
    """windows: per window its distinct sequences in order.  Per window (linked, source): linked = the set of indices whose sequence
    an earlier window held, source[index] = (window, index) of the FIRST window that held it (a later window that held it too was
    linked itself and keeps no list of its own for it)"""
    first = {}
    out = []
    for w, seqs in enumerate(windows):
        linked, source = set(), {}
        for d, read in enumerate(seqs):
            key = canonical(read)
            if key in first:
                linked.add(d)
                source[d] = first[key]
            else:
                first[key] = (w, d)
        out.append((linked, source))
    return out
