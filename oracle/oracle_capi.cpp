// oracle/oracle_capi.cpp -- TEST INFRASTRUCTURE ONLY.  Thin C ABI over the CPU restatement for ctypes-based tests.
#include <cstring>
#include "oracle_core.hpp"

using namespace t1k_oracle;

extern "C" {

// AlignAlgo::GlobalAlignment restatement.  ops must hold lent+lenp+2 bytes.  Returns the score, *nops the edit-string length.
int orc_global_alignment(const char *t, int lent, const char *p, int lenp, signed char *ops, int *nops) {
  std::vector<int8_t> v;
  int s = globalAlignment(t, lent, p, lenp, v);
  memcpy(ops, v.data(), v.size());
  *nops = (int)v.size();
  return s;
}

void *orc_create(double similarity, int relaxIntron, int maxAssign, int digitUnits, char delimiter) {
  Oracle *o = new Oracle();
  o->prm.refSeqSimilarity = similarity;
  o->prm.relaxIntronAlign = relaxIntron != 0;
  o->prm.maxAssignCnt = maxAssign;
  o->prm.alleleDigitUnits = digitUnits;
  o->prm.alleleDelimiter = delimiter;
  return o;
}
void orc_destroy(void *h) { delete (Oracle *)h; }
int orc_load_reference(void *h, const char *fasta) { return ((Oracle *)h)->loadReference(fasta); }
int orc_allele_count(void *h) { return (int)((Oracle *)h)->alleles.size(); }
const char *orc_allele_name(void *h, int i) { return ((Oracle *)h)->alleles[i].name.c_str(); }
int orc_allele_major(void *h, int i) { return ((Oracle *)h)->alleles[i].majorAllele; }  // index of its major-allele series (Genotyper::InitAlleleInfo)

// SeqSet::AssignRead restatement.  out: 12 int32 per overlap
// (seqIdx, readStart, readEnd, seqStart, seqEnd, strand, matchCnt, leftClip, rightClip, relaxedMatchCnt, simNumer, simDenom);
// sim: similarity doubles.  Returns the number of overlaps (<= cap written).
int orc_assign_read(void *h, const char *read, int weight, int *out, double *sim, int cap) {
  std::vector<Overlap> ov;
  ((Oracle *)h)->assignRead(read, weight, ov);
  int n = 0;
  for (auto &o : ov) {
    if (n >= cap) break;
    int *r = out + 12 * n;
    r[0] = o.seqIdx; r[1] = o.readStart; r[2] = o.readEnd; r[3] = o.seqStart; r[4] = o.seqEnd; r[5] = o.strand;
    r[6] = o.matchCnt; r[7] = o.leftClip; r[8] = o.rightClip; r[9] = o.relaxedMatchCnt; r[10] = 0; r[11] = 0;
    sim[n] = o.similarity;
    ++n;
  }
  return (int)ov.size();
}

// SeqSet::ReadAssignmentToFragmentAssignment + Genotyper::SetReadAssignments for one fragment.  l1 / l2: overlap lists in the layout
// orc_assign_read writes (12 int32 per overlap, similarity beside them); l2 == NULL: single-end run.  whitelist: [nAlleles] or NULL
// (Genotyper.hpp:822-823: an allele outside it is left out of the row, nothing else changes).  rowI / rowF: 3 int32 (alleleIdx, start, end)
// and 3 floats (weight, qual, adjustWeight) per row entry, at most rowCap of them written.  *fragAssigned: the list
// ReadAssignmentToFragmentAssignment returned is not empty (Genotyper.cpp:564-565).  rawI (may be NULL): that list itself, 3 int32
// (seqIdx, seqStart, seqEnd) per fragment overlap, at most rawCap written, its length in *nRaw.  Returns the number of row entries.
static void listFrom(const int *l, const double *s, int n, std::vector<Overlap> &out) {
  out.resize(n);
  for (int i = 0; i < n; ++i) {
    const int *r = l + 12 * i;
    Overlap &o = out[i];
    o.seqIdx = r[0]; o.readStart = r[1]; o.readEnd = r[2]; o.seqStart = r[3]; o.seqEnd = r[4]; o.strand = r[5];
    o.matchCnt = r[6]; o.leftClip = r[7]; o.rightClip = r[8]; o.relaxedMatchCnt = r[9];
    o.similarity = s[i];
  }
}
int orc_pair_rows(void *h, const int *l1, const double *s1, int n1, const int *l2, const double *s2, int n2, int hasN, const unsigned char *whitelist,
                  int *rowI, float *rowF, int rowCap, int *fragAssigned, int *rawI, int rawCap, int *nRaw) {
  Oracle *o = (Oracle *)h;
  std::vector<Overlap> a, b;
  listFrom(l1, s1, n1, a);
  if (l2) listFrom(l2, s2, n2, b);
  std::vector<FragmentOverlap> frag;
  o->pairFragments(a, l2 ? &b : nullptr, hasN != 0, frag);
  if (fragAssigned) *fragAssigned = frag.empty() ? 0 : 1;
  if (nRaw) *nRaw = (int)frag.size();
  if (rawI)
    for (int i = 0; i < (int)frag.size() && i < rawCap; ++i) { rawI[3 * i] = frag[i].seqIdx; rawI[3 * i + 1] = frag[i].seqStart; rawI[3 * i + 2] = frag[i].seqEnd; }
  std::vector<RowEntry> row;
  o->fragmentToRow(frag, row, whitelist);
  for (int i = 0; i < (int)row.size() && i < rowCap; ++i) {
    rowI[3 * i] = row[i].alleleIdx; rowI[3 * i + 1] = row[i].start; rowI[3 * i + 2] = row[i].end;
    rowF[3 * i] = row[i].weight; rowF[3 * i + 1] = row[i].qual; rowF[3 * i + 2] = row[i].adjustWeight;
  }
  return (int)row.size();
}

// the posting list of one k-mer (k bases of ACGT) as buildIndex made it: the alleles of its postings in list order (allele, then offset),
// at most cap of them written.  Returns the list's length, -1 for a k-mer of another length or with another letter.
int orc_kmer_postings(void *h, const char *kmer, int *alleles, int cap) {
  Oracle *o = (Oracle *)h;
  const int k = o->prm.k;
  if ((int)strlen(kmer) != k) return -1;
  uint64_t code = 0;
  for (int i = 0; i < k; ++i) {
    const char c = kmer[i];
    const int b = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1;
    if (b < 0) return -1;
    code = code << 2 | (uint64_t)b;
  }
  return o->kmerPostings(code, alleles, cap);
}

// the look-up rule of SeqSet::GetHitsFromRead as Oracle::seedHits restates it: the distinct (strand, read offset) of the hits in the
// order they were made (the read as given first; strand 0 = as given, 1 = reverse complement), the length of each one's posting list,
// and what the call added to stats.lookups / stats.postings.  At most cap entries written; returns their number.
int orc_seed_used(void *h, const char *read, int *strand, int *readOff, int *listLen, int cap, unsigned long long *lookups, unsigned long long *postings) {
  Oracle *o = (Oracle *)h;
  const uint64_t l0 = o->stats.lookups, p0 = o->stats.postings;
  std::vector<int> st, off;
  std::vector<Posting> post;
  if ((int)strlen(read) >= o->prm.k) o->seedHits(read, st, off, post);  // GetOverlapsFromRead returns before seeding a shorter read (SeqSet.hpp:1598-1599)
  if (lookups) *lookups = o->stats.lookups - l0;
  if (postings) *postings = o->stats.postings - p0;
  int n = 0;
  for (size_t i = 0; i < st.size();) {
    size_t j = i;
    while (j < st.size() && st[j] == st[i] && off[j] == off[i]) ++j;
    if (n < cap) { strand[n] = st[i] == 1 ? 0 : 1; readOff[n] = off[i]; listLen[n] = (int)(j - i); }
    ++n;
    i = j;
  }
  return n;
}

// per-base coverage of the allele's own base (the only counter GetSeqMissingBaseCoverage reads, SeqSet.hpp:2729)
int orc_coverage(void *h, int allele, int *out, int cap) {
  Oracle *o = (Oracle *)h;
  const AlleleRec &a = o->alleles[allele];
  int L = (int)a.seq.size();
  for (int i = 0; i < L && i < cap; ++i) {
    int b = a.seq[i] == 'A' ? 0 : a.seq[i] == 'C' ? 1 : a.seq[i] == 'G' ? 2 : a.seq[i] == 'T' ? 3 : -1;
    out[i] = b >= 0 ? a.cov[(size_t)i * 4 + b] : 0;
  }
  return L;
}

// Genotyper::EMupdate (Genotyper.hpp:372-421) on a table a test made: CSR over the read groups (rowPtr[nGroups + 1] into ecIdx), the groups'
// read counts, the classes' lengths.  x1 and n receive nEc doubles each; returns the sum of |x1 - x0|.
double orc_em_update(const unsigned long long *rowPtr, const unsigned *ecIdx, const double *count, const int *ecLen, unsigned nGroups, unsigned nEc,
                     const double *x0, double *x1, double *n) {
  std::vector<std::vector<int>> rows(nGroups);
  for (unsigned g = 0; g < nGroups; ++g) rows[g].assign(ecIdx + rowPtr[g], ecIdx + rowPtr[g + 1]);
  std::vector<double> c(count, count + nGroups), a(x0, x0 + nEc), b(nEc), m(nEc);
  std::vector<int> len(ecLen, ecLen + nEc);
  const double diff = Oracle::emUpdate(a, b, m, rows, c, len);
  if (nEc) { memcpy(x1, b.data(), (size_t)nEc * 8); memcpy(n, m.data(), (size_t)nEc * 8); }
  return diff;
}

// ---- candidate extraction (oracle_extract.cpp) ----
int orc_load_reference_fa(void *h, const char *fasta) { return ((Oracle *)h)->loadReferenceFa(fasta); }
int orc_infer_kmer_length(void *h) { return ((Oracle *)h)->inferKmerLength(); }
void orc_set_extract_params(void *h, int k, int hitLenRequired) {
  Oracle *o = (Oracle *)h;
  if (k != o->prm.k) o->setKmerLength(k);
  o->prm.hitLenRequired = hitLenRequired;
}
int orc_is_low_complexity(const char *read) { return Oracle::isLowComplexityRead(read) ? 1 : 0; }
int orc_has_hit_in_set(void *h, const char *read) { return ((Oracle *)h)->hasHitInSet(read) ? 1 : 0; }
int orc_is_good_candidate(void *h, const char *read) { return ((Oracle *)h)->isGoodCandidate(read) ? 1 : 0; }
}
