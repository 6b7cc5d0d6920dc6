"""The look-up rule of seeding (SeqSet::GetHitsFromRead, SeqSet.hpp:1071-1229, with strand = 0, barcode = -1, puse = NULL,
allowTotalSkip = false) in plain Python: which k-mers of a read have their posting lists used.  One of three independent statements
of the rule -- the others are Oracle::seedHits (oracle/oracle_core.cpp, through orc_seed_used) and the reference's own code
(oracle/ref_seed_harness.cpp) -- that tests/test_seed_cpu.py compares with each other and tests/test_gpu_seed.py with the kernels.

The rule, per strand (the read as given, then its reverse complement), over the k-mer positions p = 0 .. nk - 1:
  * the code of a k-mer is two bits a base, an N contributing `n_code` (nucToNum['N'] & 3: 3 in the genotyper, 0 in the extractors);
    a k-mer that holds an N is invalid and its list is empty (KmerCode::Append / KmerIndex::Search)
  * p is a look-up unless p > 0 and its code equals prevKmerCode (1104 / 1170); prevKmerCode starts as code 0 and is NOT reset
    between the strands, but position 0 of either strand is always a look-up
  * a look-up whose list has >= 100 postings and that is neither the first nor the last k-mer is skipped while skipCnt < k / 2
    (1109-1116); a skip does not update prevKmerCode (`continue`); skipCnt starts at 0 on each strand
  * any other look-up resets skipCnt and its list is used (an empty list yields no hit), and prevKmerCode is updated at every
    position that was not skipped."""

BIG = 100
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def kmers(s, k, n_code):
    """[(code, text with N replaced by the base of n_code, valid)] of every k-mer position of one strand's text"""
    sub = "ACGT"[n_code]
    out = []
    for p in range(len(s) - k + 1):
        w = s[p:p + k]
        t = w.replace("N", sub)
        c = 0
        for ch in t:
            c = c << 2 | CODE[ch]
        out.append((c, t, "N" not in w))
    return out


def breaks_precondition(read, k, n_code):
    """two equal codes within k / 2 + 1 positions of one strand: the kernels' parallel form does not apply, they replay the rule"""
    w1 = k // 2 + 1
    for s in (read, revcomp(read)):
        codes = [c for c, _, _ in kmers(s, k, n_code)]
        for p in range(len(codes)):
            if codes[p] in codes[max(0, p - w1):p]:
                return True
    return False


def seed(read, k, n_code, list_len):
    """list_len(kmer text) -> postings of its list.  Returns a dict: used = ([(offset, list length)] of the read as given, the same of the
    reverse complement), lookups, postings, replay (breaks_precondition), trace = per strand one tuple per position
    (what, list length, skipCnt before) with what in "same" (no look-up), "skip", "use", "empty" (a look-up of an empty list)."""
    used, trace = ([], []), ([], [])
    lookups = postings = 0
    if len(read) < k:  # GetOverlapsFromRead returns before seeding (1598-1599)
        return dict(used=used, lookups=0, postings=0, replay=False, trace=trace)
    prev = 0
    nk = len(read) - k + 1
    for strand, s in enumerate((read, revcomp(read))):
        skip_cnt = 0
        for p, (code, text, valid) in enumerate(kmers(s, k, n_code)):
            if p != 0 and code == prev:
                trace[strand].append(("same", None, skip_cnt))
                prev = code
                continue
            size = list_len(text) if valid else 0
            lookups += 1
            if size >= BIG and p != 0 and p != nk - 1 and skip_cnt < k // 2:
                trace[strand].append(("skip", size, skip_cnt))
                skip_cnt += 1
                continue  # prevKmerCode keeps its value
            trace[strand].append(("use" if size else "empty", size, skip_cnt))
            skip_cnt = 0
            postings += size
            if size:
                used[strand].append((p, size))
            prev = code
    return dict(used=used, lookups=lookups, postings=postings, replay=breaks_precondition(read, k, n_code), trace=trace)


def shifted_postings(res, by=1):
    """the postings the same read would count if every skipped-run choice moved by `by` positions: for each used big position that is
    neither first nor last of its strand, the neighbouring position's list instead -- what a phase error of the (k / 2 + 1) pattern
    would produce.  None when a neighbour is not a look-up of a big list (the shift is not defined there) or the read has no such position."""
    total = moved = 0
    for strand in (0, 1):
        tr = res["trace"][strand]
        for p, (what, size, _) in enumerate(tr):
            if what != "use":
                continue
            interior_big = size >= BIG and 0 < p < len(tr) - 1
            if not interior_big:
                total += size
                continue
            q = p + by
            if not (0 < q < len(tr) - 1) or tr[q][1] is None or tr[q][1] < BIG:
                return None
            total += tr[q][1]
            moved += 1
    return total if moved else None
