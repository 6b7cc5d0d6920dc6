// t1k_amd/csrc/host/analyzer.cpp -- t1k_analyzer_main(): the post-analysis stage (Analyzer.cpp:236-733 as run-t1k:438-449 starts it)
// on top of the job layer: re-assignment to the selected alleles, novel variants, per-barcode summary.
#include <cerrno>
#include <functional>
#include <numeric>
#include <tuple>
#include "job_internal.h"

extern "C" {

// ------------------------------------------------------------------------------------------------------------------
// analyzer: Analyzer.cpp:236-733 as run-t1k:438-449 starts it after the genotyper -- the aligned reads are
// assigned again, to the alleles named in <prefix>_allele.tsv only (Genotyper::InitRefSet with selectedAlleles, Genotyper.hpp:732-757;
// AssignRead with weight 0: no coverage is kept, Analyzer.cpp:139, 472), mates are paired, and BarcodeSummary (BarcodeSummary.hpp:24-80)
// turns every assigned fragment's allele list into 1/n fractional and unique counts per barcode: <prefix>_barcode_expr.tsv.
// Novel-variant calling (VariantCaller.hpp) follows as in the reference unless --varMaxGroup 0 is given (VariantCaller.hpp:980-981: no variant
// is called, <prefix>_allele.vcf is empty and AdjustFragmentAssignment hands every fragment's raw assignments back): analyzerCallVariants below.
// ------------------------------------------------------------------------------------------------------------------
// What the reference's analyzer does between its fragment assignment and its VariantCaller (Analyzer.cpp:560-684), for a job that has run its
// windows in analyzer mode (raw fragment rows resident in job->rows):
//   (1) Genotyper::SetReadAssignments + CoalesceReadAssignments + FinalizeReadAssignments + QuantifyAlleleEquivalentClass (570-609): the -n and
//       separator drops applied to the raw rows on the host, the rows coalesced (Genotyper::coalesce), the EM on the GPU (t1k_em_*) --
//       VariantCaller::SetSeqAbundance reads the alleles' abundances;
//   (2) the overlaps behind every kept assignment: the assigned fragments' distinct read-ends go through t1k_assign_batch once more on a
//       context of their own, in pieces of 32768, their final overlap lists come back (t1k_overlaps_download) and fragmentDetails takes
//       ReadAssignmentToFragmentAssignment's per-allele choice again (host/variants.cpp) -- the device rows keep the fragment's window only;
//   (3) SeqSet::AddFragmentAlignmentInfo (611-668): one global alignment per distinct (read-end, overlap) on the GPU (t1k_align_batch);
//   (4) VariantCaller::ComputeVariant on the host (host/variants.cpp).
// analyzerAlignAssignments runs (1) - (3), analyzerCallVariants (4) behind it.
struct AnalyzerVariants {
  std::vector<uint64_t> asgPtr;             // fragment -> its assignments
  std::vector<t1k_frag_assignment> asg;
  std::vector<int8_t> ops;
  std::vector<double> abundance;            // the alleles' abundances after (1)
  std::unique_ptr<VariantCaller> vc;
  int emIterations = 0;
  // T1K_DEBUG_PHASES: what (1) - (3) took
  double msRowsEM = 0, msAssign = 0, msDetails = 0, msAlign = 0;
  uint64_t nEnds = 0, nJobs = 0, nFast = 0;
};

// --pileup: the alignments of (3) booked per allele position by t1k_pileup_add, piece by piece, on the context of the
// variant pass; what comes back is the counter-major table of t1k_pileup_get
struct AnalyzerPileup {
  std::vector<uint64_t> off;       // allele -> its first position in a plane; off[A] = positions per plane
  std::vector<int32_t> counts;
  uint64_t nAln = 0, nAsg = 0, nCols = 0;  // distinct alignments walked, assignments' overlaps behind them, columns booked (weights counted)
  double msCalls = 0, msKernels = 0, msDownload = 0;
};
static const char *kPileupHeader = "#allele\tpos\texon_pos\tref\tA\tC\tG\tT\tN\tdel\tins\tA_uniq\tC_uniq\tG_uniq\tT_uniq\tN_uniq\tdel_uniq\tins_uniq\n";

// --barcodePileup: the sites are known only after VariantCaller::compute, so the piece loop of analyzerAlignAssignments keeps
// what a replay through t1k_sitepile_add needs -- per piece the pileup records, the pattern text and the booking lists (one entry
// barcode << 1 | uniq per assignment overlap that points at the record); the edit strings stay in V.ops.  Retained host memory: roughly
// the read text of the assigned fragments (once more for the read-ends with an overlap on the other strand) + 40 bytes per distinct
// alignment + 4 bytes per assignment overlap.
// --phase replays the same pieces through t1k_phase_add: its bookings are the assignments themselves, (record of mate 1,
// record of mate 2 or none, uniq), 9 more bytes per assignment.
// --siteSupport replays them through t1k_support_add: per distinct alignment its read-end's length, front clip and strand
// (12 bytes), per assignment overlap its flags and its template's extent (12 bytes, plus the 8 bytes of a list pointer per alignment).
// --indels replays them through t1k_indel_add: per distinct alignment its strand (1 byte, plus the 8 bytes of a list pointer),
// per assignment overlap whether its fragment has one assignment (1 byte).
// Any of the flags keeps the pieces; each keeps its own booking lists only.
struct AnalyzerSitepile {
  struct Piece {
    std::vector<t1k_pileup_aln> recs;
    std::string pat;
    std::vector<uint64_t> bookPtr;   // --barcodePileup
    std::vector<uint32_t> book;
    std::vector<uint32_t> asgRec;    // --phase: two per assignment, 0xFFFFFFFF = no mate
    std::vector<uint8_t> asgUniq;
    std::vector<t1k_support_rec> supRec;     // --siteSupport: one per record,
    std::vector<uint64_t> supBookPtr;        // its bookings
    std::vector<t1k_support_book> supBook;   // one per assignment overlap
    std::vector<uint8_t> indStrand;          // --indels: one per record,
    std::vector<uint64_t> indBookPtr;        // its bookings
    std::vector<uint8_t> indBookUniq;        // one per assignment overlap
    uint64_t ops0 = 0, ops1 = 0;   // the piece's edit strings: V.ops[ops0 .. ops1)
  };
  bool barcodes = false, phase = false, support = false, indels = false;    // --barcodePileup, --phase, --siteSupport, --indels
  const std::vector<int> *bcOf = nullptr;  // fragment -> barcode id (--barcodePileup)
  std::vector<Piece> pieces;
  // extra sites of --sites (allele, 0-based position), and the lines of the file that name an allele which is not selected
  std::vector<std::pair<uint32_t, uint32_t>> fileSites;
  uint64_t fileSkipped = 0;
};
// --sam: <prefix>_aligned.sam, written piece by piece inside the loop of analyzerAlignAssignments -- CIGAR, MD and NM of a
// piece's distinct alignments come from one t1k_cigar_batch, the lines are formatted per assignment behind it; nothing is retained
struct AnalyzerSam {
  FILE *fp = nullptr;
  std::string path;
  uint64_t nAln = 0, nLines = 0, cigarBytes = 0, mdBytes = 0;  // alignments encoded, lines written, bytes of the two arenas
  double msCalls = 0, msKernels = 0, msWrite = 0;
  ~AnalyzerSam() { if (fp) fclose(fp); }
};

static const char *kPhaseHeader = "#allele\tpos1\tpos2\texon_pos1\texon_pos2\tref1\tref2\tvar1\tvar2\tobs1\tobs2\tcount\tcount_uniq\n";
static const char *kSupportHeader = "#allele\tpos\texon_pos\tref\tvar\tobs\tcount\tcount_uniq\tfwd\trev\tmate1\tmate2\tend_min\tend_med\tnear_end\ttemplates\n";
static const char *kIndelHeader = "#allele\tpos\texon_pos\ttype\tlen\tseq\tcount\tcount_uniq\tfwd\trev\n";
static const char *kBarcodePileupHeader ="#barcode\tallele\tpos\texon_pos\tref\tvar\tA\tC\tG\tT\tN\tdel\tins\tA_uniq\tC_uniq\tG_uniq\tT_uniq\tN_uniq\tdel_uniq\tins_uniq\n";

// every fragment's raw row (the reference's list order): cnt[f] entries at rows[rowAt[f]]
static int analyzerRows(t1k_job *job, std::vector<uint32_t> &cnt, std::vector<uint64_t> &rowAt, std::vector<t1k_row_entry> &rows) {
  const uint32_t F = (uint32_t)job->in->nFrag();
  int rc;
  cnt.assign(F, 0);
  rowAt.assign(F + 1, 0);
  rows.clear();
  const uint32_t step = 1u << 18;
  std::vector<t1k_row_entry> part;
  for (uint32_t f0 = 0; f0 < F; f0 += step) {
    const uint32_t n = std::min(step, F - f0);
    uint64_t total = 0;
    if ((rc = t1k_rowset_rows_download(job->rows, f0, n, cnt.data() + f0, nullptr, 0, &total)) != T1K_OK) return jobFail(job, rc, t1k_rowset_last_error(job->rows));
    part.resize(total);
    if (total && (rc = t1k_rowset_rows_download(job->rows, f0, n, cnt.data() + f0, part.data(), total, &total)) != T1K_OK) return jobFail(job, rc, t1k_rowset_last_error(job->rows));
    rows.insert(rows.end(), part.begin(), part.end());
  }
  for (uint32_t f = 0; f < F; ++f) rowAt[f + 1] = rowAt[f] + cnt[f];
  if (rowAt[F] != rows.size()) return jobFail(job, T1K_ERR_INTERNAL, "analyzer: the row counts do not add up to the rows downloaded");
  return T1K_OK;
}

// step (1): the analyzer's pooled EM over the raw rows; leaves the alleles' abundances in job->ref.al[].abundance.  Used by the variant
// pass and, with --barcodeEM --barcodeEMPrior > 0 under --varMaxGroup 0, for the per-barcode EM's prior alone.
static int analyzerPooledEM(t1k_job *job, const std::vector<uint32_t> &cnt, const std::vector<uint64_t> &rowAt, const std::vector<t1k_row_entry> &rows, int *iterations) {
  const RefSet &R = job->ref;
  const uint32_t F = (uint32_t)job->in->nFrag();
  Genotyper &gt = job->gt;
  const int maxAssign = job->prm.dev.max_assign_cnt;
  std::vector<t1k_row_entry> tmp;
  for (uint32_t f = 0; f < F; ++f) {
    const uint32_t k = cnt[f];
    if (!k || (maxAssign > 0 && (int)k > maxAssign)) continue;  // Genotyper.hpp:783-784
    bool sep = false;                                            // IsFragmentSpanSeparator (796-800): an N of the allele inside the fragment's window
    for (uint32_t j = 0; j < k && !sep; ++j) {
      const t1k_row_entry &e = rows[rowAt[f] + j];
      const std::string &sq = R.seqs[e.allele_idx];
      for (int p = std::max(e.start, 0); p <= e.end && p < (int)sq.size(); ++p)
        if (sq[p] == 'N') { sep = true; break; }
    }
    if (sep) continue;
    tmp.assign(rows.begin() + rowAt[f], rows.begin() + rowAt[f] + k);
    gt.coalesce(tmp.data(), k, f);
  }
  gt.finalize(std::vector<int32_t>(R.al.size(), 0));  // (missingCoverage is not read before selection, which the analyzer does not run)
  *iterations = 0;
  if (gt.nGroups() && (*iterations = gt.quantify(job->ctx, nullptr, job->err)) < 0) return T1K_ERR_DEVICE;
  return T1K_OK;
}

// steps (1) - (3): V.asgPtr / V.asg / V.ops and V.abundance; with `pile`, every piece's alignments go through t1k_pileup_add as well; with `sp`,
// every piece's records, pattern text and booking lists are kept for analyzerSitepile; with `sam`, every piece's alignments go through
// t1k_cigar_batch and its assignments' lines into the open file
static int analyzerAlignAssignments(t1k_job *job, AnalyzerVariants &V, AnalyzerPileup *pile, AnalyzerSitepile *sp = nullptr, AnalyzerSam *sam = nullptr) {
  const double tv0 = nowMs();
  double &msAssign = V.msAssign, &msDetails = V.msDetails, &msAlign = V.msAlign;
  uint64_t &nEnds = V.nEnds, &nJobs = V.nJobs, &nFast = V.nFast;
  const ReadInput &in = *job->in;
  const RefSet &R = job->ref;
  const uint32_t F = (uint32_t)in.nFrag();
  const bool paired = in.paired;
  int rc;
  std::vector<uint32_t> cnt;
  std::vector<uint64_t> rowAt;
  std::vector<t1k_row_entry> rows;
  if ((rc = analyzerRows(job, cnt, rowAt, rows)) != T1K_OK) return rc;
  // (1) the analyzer's EM
  if ((rc = analyzerPooledEM(job, cnt, rowAt, rows, &V.emIterations)) != T1K_OK) return rc;
  V.abundance.resize(R.al.size());
  for (size_t a = 0; a < R.al.size(); ++a) V.abundance[a] = R.al[a].abundance;
  V.msRowsEM = nowMs() - tv0;
  // (2) + (3)
  t1k_ctx *vctx = nullptr;
  if ((rc = t1k_ctx_create(job->prm.device, &job->prm.dev, &vctx)) != T1K_OK) { if (vctx) t1k_ctx_destroy(vctx); return jobFail(job, rc, "analyzer: cannot create the context of the variant pass"); }
  struct CtxGuard { t1k_ctx *c; ~CtxGuard() { t1k_ctx_destroy(c); } } guard{vctx};
  if ((rc = t1k_ref_share(vctx, job->ctx)) != T1K_OK) return jobFail(job, rc, t1k_last_error(vctx));
  std::string refText;
  std::vector<uint64_t> refOff(R.seqs.size() + 1, 0);
  for (size_t a = 0; a < R.seqs.size(); ++a) refOff[a + 1] = refOff[a] + R.seqs[a].size();
  if (refOff.back() >= (1ull << 32)) return jobFail(job, T1K_ERR_CAPACITY, "analyzer: the selected alleles hold more than 4 G bases");
  refText.reserve(refOff.back());
  for (const std::string &sq : R.seqs) refText += sq;
  if (pile && (rc = t1k_pileup_begin(vctx, (uint32_t)R.seqs.size(), refOff.data())) != T1K_OK) return jobFail(job, rc, std::string("analyzer: ") + t1k_last_error(vctx));
  V.asgPtr.assign(F + 1, 0);
  V.asg.resize(rows.size());
  for (uint32_t f = 0; f < F; ++f) V.asgPtr[f + 1] = V.asgPtr[f] + (job->fragAssigned[f] ? cnt[f] : 0);
  V.asg.resize(V.asgPtr[F]);
  // read-ends per piece: the range size of the job's own loop (T1K_ANALYZER_PIECE: tests run several pieces on small inputs)
  const uint32_t pieceEnds = getenv("T1K_ANALYZER_PIECE") ? (uint32_t)std::max(2, atoi(getenv("T1K_ANALYZER_PIECE"))) : 32768u;
  auto readOf = [&](uint32_t f, int m) { const uint32_t r = in.frag[f]; return std::pair<const char *, uint32_t>(in.side[m].seqP[r], in.side[m].seqL[r]); };
  uint32_t f0 = 0;
  while (f0 < F) {
    // a piece: fragments [f0, f1) whose distinct read-ends fit one upload
    // (identical read-ends of the piece are assigned once: an open-addressing table over a 64-bit hash of the bases, membership decided by comparing
    // the bases themselves -- the std::unordered_map<std::string, ...> of round 5 allocated a string per read-end: 0.4 s per million pairs)
    std::vector<std::pair<const char *, uint32_t>> ends;
    size_t slots = 64;
    while (slots < (size_t)pieceEnds * 4) slots <<= 1;
    std::vector<uint32_t> table(slots, ~0u);
    auto endId = [&](const char *p, uint32_t n) -> uint32_t {
      uint64_t h = 0x9E3779B97F4A7C15ull ^ n;
      uint32_t i = 0;
      for (; i + 8 <= n; i += 8) { uint64_t w; memcpy(&w, p + i, 8); h = (h ^ w) * 0xD6E8FEB86659FD93ull; h ^= h >> 29; }
      for (; i < n; ++i) { h = (h ^ (uint8_t)p[i]) * 0x100000001B3ull; }
      h ^= h >> 32;
      for (size_t q = (size_t)h & (slots - 1);; q = (q + 1) & (slots - 1)) {
        const uint32_t e = table[q];
        if (e == ~0u) { table[q] = (uint32_t)ends.size(); ends.emplace_back(p, n); return (uint32_t)ends.size() - 1; }
        if (ends[e].second == n && memcmp(ends[e].first, p, n) == 0) return e;
      }
    };
    std::vector<uint32_t> endOf;  // (fragment - f0) * 2 + mate -> distinct read-end of the piece
    uint32_t f1 = f0;
    for (; f1 < F && ends.size() + 2 <= pieceEnds; ++f1) {
      endOf.push_back(~0u); endOf.push_back(~0u);
      if (!job->fragAssigned[f1] || !cnt[f1]) continue;
      for (int m = 0; m < (paired ? 2 : 1); ++m) {
        auto rd = readOf(f1, m);
        endOf[(size_t)(f1 - f0) * 2 + m] = endId(rd.first, rd.second);
      }
    }
    const uint32_t E = (uint32_t)ends.size();
    if (E) {
      std::string text;
      std::vector<uint64_t> off(E + 1, 0);
      for (uint32_t e = 0; e < E; ++e) off[e + 1] = off[e] + ends[e].second;
      text.reserve(off[E]);
      for (uint32_t e = 0; e < E; ++e) text.append(ends[e].first, ends[e].second);
      const double ta = nowMs();
      nEnds += E;
      if ((rc = t1k_reads_upload(vctx, text.data(), off.data(), nullptr, E)) != T1K_OK) return jobFail(job, rc, t1k_last_error(vctx));
      if ((rc = t1k_assign_batch(vctx)) != T1K_OK) return jobFail(job, rc, t1k_last_error(vctx));
      std::vector<uint32_t> lc(E);
      uint64_t total = 0;
      if ((rc = t1k_overlaps_download(vctx, lc.data(), nullptr, 0, &total)) != T1K_OK) return jobFail(job, rc, t1k_last_error(vctx));
      std::vector<t1k_overlap> lists(total);
      if (total && (rc = t1k_overlaps_download(vctx, lc.data(), lists.data(), total, &total)) != T1K_OK) return jobFail(job, rc, t1k_last_error(vctx));
      std::vector<uint64_t> listAt(E + 1, 0);
      for (uint32_t e = 0; e < E; ++e) listAt[e + 1] = listAt[e] + lc[e];
      const double tb = nowMs();
      msAssign += tb - ta;
      // the overlaps behind every kept assignment, and where each of them sits in its read-end's list (found again by its coordinates): per
      // fragment, by the host threads (round 6); the alignment jobs -- one per distinct (read-end, overlap) -- are numbered behind them in
      // fragment order, as before
      const uint64_t q0 = V.asgPtr[f0], nAsg = V.asgPtr[f1] - q0;
      std::vector<int64_t> at[2];   // assignment -> index of its overlap(s) in `lists`
      at[0].assign(nAsg, -1); at[1].assign(nAsg, -1);
      std::atomic<int64_t> badFrag{-1};
      std::atomic<int> badKind{0};
      parallelRanges((size_t)(f1 - f0), hostThreads(job), [&](int, size_t lo, size_t hi) {
        std::vector<int32_t> alleles;
        auto find = [&](uint32_t e, const t1k_overlap &o) -> int64_t {
          for (uint32_t i = 0; i < lc[e]; ++i) {
            const t1k_overlap &c = lists[listAt[e] + i];
            if (c.seq_idx == o.seq_idx && c.read_start == o.read_start && c.read_end == o.read_end && c.seq_start == o.seq_start && c.seq_end == o.seq_end && c.strand == o.strand)
              return (int64_t)(listAt[e] + i);
          }
          return -1;
        };
        for (size_t x = lo; x < hi; ++x) {
          const uint32_t f = f0 + (uint32_t)x;
          if (!job->fragAssigned[f] || !cnt[f]) continue;
          const uint32_t k = cnt[f];
          alleles.resize(k);
          for (uint32_t j = 0; j < k; ++j) alleles[j] = rows[rowAt[f] + j].allele_idx;
          const uint32_t e1 = endOf[x * 2], e2 = paired ? endOf[x * 2 + 1] : 0;
          if (!fragmentDetails(lists.data() + listAt[e1], lc[e1], paired ? lists.data() + listAt[e2] : nullptr, paired ? lc[e2] : 0, paired, alleles.data(), k, V.asg.data() + V.asgPtr[f])) {
            badKind = 1; badFrag = f; return;
          }
          for (uint64_t q = V.asgPtr[f]; q < V.asgPtr[f + 1]; ++q) {
            const t1k_frag_assignment &a = V.asg[q];
            const uint32_t eA = endOf[x * 2 + ((a.o1_from_r2 && !a.has_mate_pair) ? 1 : 0)];
            if ((at[0][q - q0] = find(eA, a.o1)) < 0 || (a.has_mate_pair && (at[1][q - q0] = find(endOf[x * 2 + 1], a.o2)) < 0)) { badKind = 2; badFrag = f; return; }
          }
        }
      });
      if (badKind.load() == 1) return jobFail(job, T1K_ERR_INTERNAL, "analyzer: fragment " + std::to_string(badFrag.load()) + " is assigned to an allele its read-ends' overlap lists do not hold");
      if (badKind.load() == 2) return jobFail(job, T1K_ERR_INTERNAL, "analyzer: an assignment's overlap is not in its read-end's list");
      std::vector<int64_t> jobOf(total, -1);
      struct Job { uint32_t end, idx; };
      std::vector<Job> jobs;
      std::vector<uint32_t> endOfList(total);   // list entry -> its read-end
      for (uint32_t e = 0; e < E; ++e) for (uint64_t i = listAt[e]; i < listAt[e + 1]; ++i) endOfList[i] = e;
      std::vector<int64_t> jobOfAsg[2];
      jobOfAsg[0].assign(nAsg, -1);
      jobOfAsg[1].assign(nAsg, -1);
      for (uint64_t q = 0; q < nAsg; ++q)
        for (int m = 0; m < 2; ++m) {
          const int64_t li = at[m][q];
          if (li < 0) continue;
          int64_t &slot = jobOf[li];
          if (slot < 0) { slot = (int64_t)jobs.size(); jobs.push_back({endOfList[li], (uint32_t)(li - (int64_t)listAt[endOfList[li]])}); }
          jobOfAsg[m][q] = slot;
        }
      // patterns: the read-ends as they are and, where an overlap is on the other strand, reverse-complemented (SeqSet.hpp:2663-2668)
      std::vector<uint64_t> rcAt(E, ~0ull);
      std::string pat = text;
      for (const Job &jb : jobs)
        if (lists[listAt[jb.end] + jb.idx].strand == -1 && rcAt[jb.end] == ~0ull) {
          rcAt[jb.end] = pat.size();
          const char *p = ends[jb.end].first;
          const uint32_t n = ends[jb.end].second;
          for (uint32_t i = 0; i < n; ++i) { const char c = p[n - 1 - i]; pat += c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N'; }
        }
      if (pat.size() >= (1ull << 32)) return jobFail(job, T1K_ERR_CAPACITY, "analyzer: a piece's read text exceeds 4 GB");
      std::vector<uint64_t> opsAtOfJob(jobs.size());
      std::vector<uint32_t> nOpsOfJob(jobs.size());
      const double tc = nowMs();
      msDetails += tc - tb;
      nJobs += jobs.size();
      // Round 6: most of these alignments never reach the device.  Text and pattern of equal length with at most two mismatches ('N' on
      // either side matches, AlignAlgo.hpp:304-305): the ungapped alignment scores 2L - 4x >= 2L - 8, anything with a gap at most 2L - 12 (one
      // insertion AND one deletion at least) -- the diagonal is the strict optimum at every prefix, and the reference's traceback takes the
      // diagonal wherever it attains the cell (AlignAlgo.hpp:335-343): the edit string is MATCH / MISMATCH by position (checked against
      // the reference's routine on 232 363 cases).  The host threads write those strings straight into the job's edit-string store; what is
      // left (reads with an indel or three and more mismatches: a few per cent) goes through t1k_align_batch as before.  T1K_ANALYZER_NO_FAST=1:
      // everything through the device (A/B and the test that both ways agree).
      static const bool noFast = getenv("T1K_ANALYZER_NO_FAST") != nullptr;
      const size_t nJ = jobs.size();
      std::vector<uint32_t> jT(nJ), jTL(nJ), jP(nJ), jPL(nJ);
      std::vector<uint8_t> fast(nJ, 0);
      const int TH = hostThreads(job);
      parallelRanges(nJ, TH, [&](int, size_t lo, size_t hi) {
        for (size_t j = lo; j < hi; ++j) {
          const Job &jb = jobs[j];
          const t1k_overlap &o = lists[listAt[jb.end] + jb.idx];
          jT[j] = (uint32_t)(refOff[o.seq_idx] + (uint64_t)o.seq_start);
          jTL[j] = (uint32_t)(o.seq_end - o.seq_start + 1);
          jP[j] = (uint32_t)((o.strand == -1 ? rcAt[jb.end] : off[jb.end]) + (uint64_t)o.read_start);
          jPL[j] = (uint32_t)(o.read_end - o.read_start + 1);
          if (noFast || jTL[j] != jPL[j]) continue;
          const char *t = refText.data() + jT[j], *q = pat.data() + jP[j];
          int x = 0;
          for (uint32_t i = 0; i < jTL[j] && x <= 2; ++i) x += (t[i] != q[i] && t[i] != 'N' && q[i] != 'N') ? 1 : 0;
          fast[j] = x <= 2;
        }
      });
      // the rest: through the device, in calls of at most 2^18
      std::vector<uint32_t> slow;
      for (size_t j = 0; j < nJ; ++j) if (!fast[j]) slow.push_back((uint32_t)j);
      std::vector<std::vector<int8_t>> slowBuf;
      std::vector<uint32_t> slowOff(slow.size()), slowCall(slow.size());
      const size_t callJobs = 1u << 18;
      for (size_t j0 = 0; j0 < slow.size(); j0 += callJobs) {
        const uint32_t n = (uint32_t)std::min(callJobs, slow.size() - j0);
        std::vector<uint32_t> tOff(n), tLen(n), pOff(n), pLen(n), oOff(n), nOps(n);
        uint64_t room = 0;
        for (uint32_t i = 0; i < n; ++i) {
          const uint32_t j = slow[j0 + i];
          tOff[i] = jT[j]; tLen[i] = jTL[j]; pOff[i] = jP[j]; pLen[i] = jPL[j];
          oOff[i] = (uint32_t)room;
          room += (uint64_t)tLen[i] + pLen[i] + 2;
        }
        if (room >= (1ull << 32)) return jobFail(job, T1K_ERR_CAPACITY, "analyzer: the edit strings of one alignment call exceed 4 GB");
        slowBuf.emplace_back(room + 64);
        if ((rc = t1k_align_batch(vctx, refText.data(), tOff.data(), tLen.data(), pat.data(), pOff.data(), pLen.data(), n, nullptr, nullptr, nullptr, nullptr, slowBuf.back().data(), oOff.data(), nOps.data())) != T1K_OK)
          return jobFail(job, rc, t1k_last_error(vctx));
        for (uint32_t i = 0; i < n; ++i) { nOpsOfJob[slow[j0 + i]] = nOps[i]; slowOff[j0 + i] = oOff[i]; slowCall[j0 + i] = (uint32_t)(slowBuf.size() - 1); }
      }
      // every job's place in the store (job order, as before), then the strings, by the host threads
      const uint64_t pieceOps0 = V.ops.size();
      {
        uint64_t at = V.ops.size();
        for (size_t j = 0; j < nJ; ++j) { if (fast[j]) nOpsOfJob[j] = jTL[j]; opsAtOfJob[j] = at; at += nOpsOfJob[j]; }
        V.ops.resize(at);
        std::vector<uint32_t> slowIdx(nJ, 0);
        for (size_t i = 0; i < slow.size(); ++i) slowIdx[slow[i]] = (uint32_t)i;
        int8_t *store = V.ops.data();
        parallelRanges(nJ, TH, [&](int, size_t lo, size_t hi) {
          for (size_t j = lo; j < hi; ++j) {
            int8_t *dst = store + opsAtOfJob[j];
            if (fast[j]) {
              const char *t = refText.data() + jT[j], *q = pat.data() + jP[j];
              for (uint32_t i = 0; i < jTL[j]; ++i) dst[i] = (t[i] != q[i] && t[i] != 'N' && q[i] != 'N') ? 1 : 0;   // EDIT_MISMATCH : EDIT_MATCH (AlignAlgo.hpp:7-8)
            } else {
              const uint32_t i = slowIdx[j];
              memcpy(dst, slowBuf[slowCall[i]].data() + slowOff[i], nOpsOfJob[j]);
            }
          }
        });
      }
      nFast += nJ - slow.size();
      for (uint64_t q = V.asgPtr[f0]; q < V.asgPtr[f1]; ++q) {
        t1k_frag_assignment &a = V.asg[q];
        const int64_t j1 = jobOfAsg[0][q - V.asgPtr[f0]], j2 = jobOfAsg[1][q - V.asgPtr[f0]];
        a.ops1 = opsAtOfJob[j1]; a.n_ops1 = nOpsOfJob[j1];
        if (a.has_mate_pair) { a.ops2 = opsAtOfJob[j2]; a.n_ops2 = nOpsOfJob[j2]; }
      }
      msAlign += nowMs() - tc;
      // one record per alignment job, for --sam and for the pileups (which count its weights below)
      std::vector<t1k_pileup_aln> recs((pile || sp || sam) ? nJ : 0);
      for (size_t j = 0; j < recs.size(); ++j) {
        const t1k_overlap &o = lists[listAt[jobs[j].end] + jobs[j].idx];
        recs[j] = t1k_pileup_aln{(uint32_t)o.seq_idx, (uint32_t)o.seq_start, jP[j], opsAtOfJob[j] - pieceOps0, nOpsOfJob[j], 0, 0, 0};
      }
      if (sam && nJ) {
        // every job's clips from its read window; then one line per assignment overlap, in fragment order
        const double ts = nowMs();
        std::vector<uint32_t> clip(2 * nJ);
        uint64_t cigarCap = 0, mdCap = 0;
        for (size_t j = 0; j < nJ; ++j) {
          const t1k_overlap &o = lists[listAt[jobs[j].end] + jobs[j].idx];
          clip[2 * j] = (uint32_t)o.read_start;
          clip[2 * j + 1] = ends[jobs[j].end].second - 1u - (uint32_t)o.read_end;
          cigarCap += 2ull * nOpsOfJob[j] + 22;  // the bounds of t1k_cigar_batch (include/t1k_gpu.h)
          mdCap += 3ull * nOpsOfJob[j] + 11;
        }
        std::vector<uint64_t> cigarPtr(nJ + 1), mdPtr(nJ + 1);
        std::vector<char> cigar(cigarCap), md(mdCap);
        std::vector<uint32_t> nm(nJ), span(nJ);
        double kernelMs = 0;
        if ((rc = t1k_cigar_batch(vctx, recs.data(), (uint32_t)nJ, clip.data(), V.ops.data() + pieceOps0, V.ops.size() - pieceOps0, (uint32_t)R.seqs.size(), refOff.data(), refText.data(),
                                  cigarPtr.data(), cigar.data(), cigarCap, mdPtr.data(), md.data(), mdCap, nm.data(), span.data(), &kernelMs)) != T1K_OK)
          return jobFail(job, rc, std::string("analyzer: ") + t1k_last_error(vctx));
        const double tw = nowMs();
        sam->nAln += nJ; sam->cigarBytes += cigarPtr[nJ]; sam->mdBytes += mdPtr[nJ];
        sam->msKernels += kernelMs; sam->msCalls += tw - ts;
        std::string out;
        char num[96];
        bool wrote = true;
        for (uint32_t f = f0; f < f1; ++f) {
          const uint64_t k = V.asgPtr[f + 1] - V.asgPtr[f];
          const int mapq = k == 1 ? 60 : k == 2 ? 3 : k <= 4 ? 1 : 0;
          const uint32_t r = in.frag[f];
          for (uint64_t q = V.asgPtr[f]; q < V.asgPtr[f + 1]; ++q) {
            const t1k_frag_assignment &a = V.asg[q];
            const int64_t js[2] = {jobOfAsg[0][q - q0], jobOfAsg[1][q - q0]};
            for (int m = 0; m < 2; ++m) {
              const int64_t j = js[m];
              if (j < 0) continue;
              const t1k_overlap &o = lists[listAt[jobs[j].end] + jobs[j].idx];
              const bool second = m == 1 || (a.o1_from_r2 && !a.has_mate_pair);  // the line's read-end is read 2
              int flag = (paired ? 0x1 : 0) | (o.strand == -1 ? 0x10 : 0) | (q > V.asgPtr[f] ? 0x100 : 0);
              long long pnext = 0, tlen = 0;
              if (a.has_mate_pair) {
                const int64_t jm = js[1 - m];
                const t1k_overlap &om = lists[listAt[jobs[jm].end] + jobs[jm].idx];
                flag |= 0x2 | (m == 0 ? 0x40 : 0x80) | (om.strand == -1 ? 0x20 : 0);
                pnext = (long long)om.seq_start + 1;
                const long long left = std::min<long long>(o.seq_start, om.seq_start);
                const long long right = std::max<long long>((long long)o.seq_start + span[j], (long long)om.seq_start + span[jm]);  // one behind the rightmost mapped base
                tlen = right - left;
                if (o.seq_start > om.seq_start || (o.seq_start == om.seq_start && m == 1)) tlen = -tlen;
              } else if (paired) flag |= 0x8 | (second ? 0x80 : 0x40);
              if (in.noIds) { snprintf(num, sizeof num, "r%u", f); out += num; }
              else out.append(in.side[0].idP[r], in.side[0].idL[r]);
              snprintf(num, sizeof num, "\t%d\t", flag);
              out += num;
              out += R.al[o.seq_idx].name;
              snprintf(num, sizeof num, "\t%lld\t%d\t", (long long)o.seq_start + 1, mapq);
              out += num;
              out.append(cigar.data() + cigarPtr[j], cigarPtr[j + 1] - cigarPtr[j]);
              snprintf(num, sizeof num, a.has_mate_pair ? "\t=\t%lld\t%lld\t" : "\t*\t%lld\t%lld\t", pnext, tlen);
              out += num;
              out.append(pat.data() + (o.strand == -1 ? rcAt[jobs[j].end] : off[jobs[j].end]), ends[jobs[j].end].second);  // the whole read-end, strand-corrected
              snprintf(num, sizeof num, "\t*\tNM:i:%u\tMD:Z:", nm[j]);
              out += num;
              out.append(md.data() + mdPtr[j], mdPtr[j + 1] - mdPtr[j]);
              snprintf(num, sizeof num, "\tNH:i:%llu\tHI:i:%llu\n", (unsigned long long)k, (unsigned long long)(q - V.asgPtr[f] + 1));
              out += num;
              ++sam->nLines;
            }
          }
          if (out.size() >= (1u << 20)) { wrote = wrote && fwrite(out.data(), 1, out.size(), sam->fp) == out.size(); out.clear(); }
        }
        wrote = wrote && fwrite(out.data(), 1, out.size(), sam->fp) == out.size();
        if (!wrote) return jobFail(job, T1K_ERR_IO, "analyzer: cannot write " + sam->path);
        sam->msWrite += nowMs() - tw;
      }
      if ((pile || sp) && nJ) {
        // a record's weights = the assignments that point at it, and those of them whose fragment keeps one assignment
        const double tp = nowMs();
        for (uint32_t f = f0; f < f1; ++f) {
          const bool one = V.asgPtr[f + 1] - V.asgPtr[f] == 1;
          for (uint64_t q = V.asgPtr[f]; q < V.asgPtr[f + 1]; ++q) {
            const t1k_frag_assignment &a = V.asg[q];
            if (a.o1.seq_idx != a.allele_idx || (a.has_mate_pair && a.o2.seq_idx != a.allele_idx))
              return jobFail(job, T1K_ERR_INTERNAL, "analyzer: an assignment's overlap lies on another allele than the assignment");
            for (int m = 0; m < 2; ++m) {
              const int64_t j = jobOfAsg[m][q - q0];
              if (j < 0) continue;
              ++recs[j].w_all;
              if (one) ++recs[j].w_uniq;
              if (pile) { ++pile->nAsg; pile->nCols += nOpsOfJob[j]; }
            }
          }
        }
        if (pile) {
          double kernelMs = 0;
          if ((rc = t1k_pileup_add(vctx, recs.data(), (uint32_t)nJ, pat.data(), pat.size(), V.ops.data() + pieceOps0, V.ops.size() - pieceOps0, &kernelMs)) != T1K_OK)
            return jobFail(job, rc, std::string("analyzer: ") + t1k_last_error(vctx));
          pile->nAln += nJ;
          pile->msKernels += kernelMs;
          pile->msCalls += nowMs() - tp;
        }
        if (sp) {
          // the same loop once more, now that every record's number of bookings (w_all) is known: its list, in fragment order
          AnalyzerSitepile::Piece pc;
          std::vector<uint64_t> fill;
          if (sp->barcodes) {
            pc.bookPtr.assign(nJ + 1, 0);
            for (size_t j = 0; j < nJ; ++j) pc.bookPtr[j + 1] = pc.bookPtr[j] + recs[j].w_all;
            pc.book.resize(pc.bookPtr[nJ]);
            fill.assign(pc.bookPtr.begin(), pc.bookPtr.end() - 1);
          }
          if (sp->phase) { pc.asgRec.reserve(2 * nAsg); pc.asgUniq.reserve(nAsg); }
          std::vector<uint64_t> supFill;
          if (sp->support) {
            // per record what AnalyzerSam takes its clips and flag 0x10 from: the read-end's length, the bases in front of the window (in the
            // strand-corrected read-end, which is what `pat` holds) and the strand
            pc.supRec.resize(nJ);
            pc.supBookPtr.assign(nJ + 1, 0);
            for (size_t j = 0; j < nJ; ++j) {
              const t1k_overlap &o = lists[listAt[jobs[j].end] + jobs[j].idx];
              pc.supRec[j] = t1k_support_rec{ends[jobs[j].end].second, (uint32_t)o.read_start, o.strand == -1 ? 1u : 0u};
              pc.supBookPtr[j + 1] = pc.supBookPtr[j] + recs[j].w_all;
            }
            pc.supBook.resize(pc.supBookPtr[nJ]);
            supFill.assign(pc.supBookPtr.begin(), pc.supBookPtr.end() - 1);
          }
          std::vector<uint64_t> indFill;
          if (sp->indels) {
            // per record the strand, from where supRec takes it
            pc.indStrand.resize(nJ);
            pc.indBookPtr.assign(nJ + 1, 0);
            for (size_t j = 0; j < nJ; ++j) {
              pc.indStrand[j] = lists[listAt[jobs[j].end] + jobs[j].idx].strand == -1 ? 1 : 0;
              pc.indBookPtr[j + 1] = pc.indBookPtr[j] + recs[j].w_all;
            }
            pc.indBookUniq.resize(pc.indBookPtr[nJ]);
            indFill.assign(pc.indBookPtr.begin(), pc.indBookPtr.end() - 1);
          }
          for (uint32_t f = f0; f < f1; ++f) {
            const uint32_t one = V.asgPtr[f + 1] - V.asgPtr[f] == 1 ? 1u : 0u;
            for (uint64_t q = V.asgPtr[f]; q < V.asgPtr[f + 1]; ++q) {
              if (sp->indels)
                for (int m = 0; m < 2; ++m) {
                  const int64_t j = jobOfAsg[m][q - q0];
                  if (j >= 0) pc.indBookUniq[indFill[j]++] = (uint8_t)one;
                }
              if (sp->support) {
                // the template of the assignment: both mates' extent on the allele, and which way the fragment lies (file 1 on the reverse
                // strand; with a file-2 read-end alone, that one on the forward strand)
                const t1k_frag_assignment &a = V.asg[q];
                const bool pairHere = a.has_mate_pair != 0, from2 = a.o1_from_r2 && !pairHere;
                const uint32_t tStart = (uint32_t)(pairHere ? std::min(a.o1.seq_start, a.o2.seq_start) : a.o1.seq_start);
                const uint32_t tEnd = (uint32_t)(pairHere ? std::max(a.o1.seq_end, a.o2.seq_end) : a.o1.seq_end);
                const uint32_t orient = (from2 ? a.o1.strand == 1 : a.o1.strand == -1) ? 1u : 0u;
                for (int m = 0; m < 2; ++m) {
                  const int64_t j = jobOfAsg[m][q - q0];
                  if (j < 0) continue;
                  const uint32_t second = (m == 1 || from2) ? 1u : 0u;  // the read-end is read 2, as AnalyzerSam's `second`
                  pc.supBook[supFill[j]++] = t1k_support_book{one | (second << 1) | (orient << 2), tStart, tEnd};
                }
              }
              if (sp->barcodes)
                for (int m = 0; m < 2; ++m) {
                  const int64_t j = jobOfAsg[m][q - q0];
                  if (j >= 0) pc.book[fill[j]++] = ((uint32_t)(*sp->bcOf)[f] << 1) | one;
                }
              if (sp->phase) {
                const int64_t j1 = jobOfAsg[0][q - q0], j2 = jobOfAsg[1][q - q0];
                pc.asgRec.push_back((uint32_t)j1);
                pc.asgRec.push_back(j2 >= 0 ? (uint32_t)j2 : 0xFFFFFFFFu);
                pc.asgUniq.push_back((uint8_t)one);
              }
            }
          }
          pc.recs = std::move(recs);
          pc.pat = std::move(pat);
          pc.ops0 = pieceOps0; pc.ops1 = V.ops.size();
          sp->pieces.push_back(std::move(pc));
        }
      }
    }
    f0 = f1;
  }
  if (pile) {
    const double tp = nowMs();
    pile->off = refOff;
    pile->counts.assign((size_t)14 * refOff.back(), 0);
    if ((rc = t1k_pileup_get(vctx, pile->counts.data())) != T1K_OK || (rc = t1k_pileup_end(vctx)) != T1K_OK) return jobFail(job, rc, std::string("analyzer: ") + t1k_last_error(vctx));
    pile->msDownload = nowMs() - tp;
  }
  return T1K_OK;
}

static int analyzerCallVariants(t1k_job *job, int varMaxGroup, AnalyzerVariants &V, AnalyzerPileup *pile, AnalyzerSitepile *sp, AnalyzerSam *sam) {
  const double tv0 = nowMs();
  int rc;
  if ((rc = analyzerAlignAssignments(job, V, pile, sp, sam)) != T1K_OK) return rc;
  const ReadInput &in = *job->in;
  const RefSet &R = job->ref;
  const uint32_t F = (uint32_t)in.nFrag();
  const bool paired = in.paired;
  auto readOf = [&](uint32_t f, int m) { const uint32_t r = in.frag[f]; return std::pair<const char *, uint32_t>(in.side[m].seqP[r], in.side[m].seqL[r]); };
  const double tv2 = nowMs();
  // (4)
  std::vector<VariantCaller::Fragment> frags(F);
  for (uint32_t f = 0; f < F; ++f) {
    VariantCaller::Fragment &fr = frags[f];
    fr.asg = V.asg.data() + V.asgPtr[f];
    fr.n = (uint32_t)(V.asgPtr[f + 1] - V.asgPtr[f]);
    auto a = readOf(f, 0);
    fr.r1 = a.first; fr.l1 = a.second;
    if (paired) { auto b = readOf(f, 1); fr.r2 = b.first; fr.l2 = b.second; }
  }
  V.vc.reset(new VariantCaller(R, V.abundance, varMaxGroup));
  V.vc->compute(frags, V.ops.data());
  if (getenv("T1K_DEBUG_PHASES"))
    fprintf(stderr, "[t1k analyzer] variant pass: rows + EM %.1f ms; %llu distinct read-ends re-assigned in %.1f ms, overlaps chosen in %.1f ms, %llu alignments (%llu of them on the host: equal lengths, at most two mismatches) in %.1f ms; "
                    "VariantCaller %.1f ms (%zu assignments, %zu variants); %.1f ms in all\n", V.msRowsEM, (unsigned long long)V.nEnds, V.msAssign, V.msDetails, (unsigned long long)V.nJobs, (unsigned long long)V.nFast, V.msAlign,
            nowMs() - tv2, V.asg.size(), V.vc->variants.size(), nowMs() - tv0);
  return T1K_OK;
}

// <prefix>_allele_pileup.tsv: one line per base of every selected allele, in job->ref.al order.  pile == NULL: the header alone
static bool analyzerWritePileup(t1k_job *job, const std::string &prefix, AnalyzerPileup *pile) {
  const double t0 = nowMs();
  FILE *fp = fopen((prefix + "_allele_pileup.tsv").c_str(), "w");
  if (!fp) { fprintf(stderr, "analyzer: cannot write %s_allele_pileup.tsv\n", prefix.c_str()); return false; }
  fputs(kPileupHeader, fp);
  if (pile) {
    const RefSet &R = job->ref;
    const uint64_t T = pile->off.back();
    std::string out;
    char num[32];
    for (size_t a = 0; a < R.seqs.size(); ++a) {
      const std::string &sq = R.seqs[a];
      int exonic = 0;  // exonic bases in front of the position (SeqSet::GetExonicPosition)
      for (size_t pos = 0; pos < sq.size(); ++pos) {
        out += R.al[a].name;
        snprintf(num, sizeof num, "\t%zu\t", pos + 1);
        out += num;
        if (R.exon[a][pos]) { snprintf(num, sizeof num, "%d", ++exonic); out += num; } else out += '.';
        out += '\t';
        out += sq[pos];
        for (int c = 0; c < 14; ++c) { snprintf(num, sizeof num, "\t%d", pile->counts[(size_t)c * T + pile->off[a] + pos]); out += num; }
        out += '\n';
        if (out.size() >= (1u << 20)) { fwrite(out.data(), 1, out.size(), fp); out.clear(); }
      }
    }
    fwrite(out.data(), 1, out.size(), fp);
  }
  fclose(fp);
  if (pile && getenv("T1K_DEBUG_PHASES"))
    fprintf(stderr, "pileup: %llu alignments walked, %llu assignments behind them, %llu columns booked; upload %.1f ms, kernels %.1f ms, download + write %.1f ms\n",
            (unsigned long long)pile->nAln, (unsigned long long)pile->nAsg, (unsigned long long)pile->nCols, std::max(0.0, pile->msCalls - pile->msKernels), pile->msKernels,
            pile->msDownload + (nowMs() - t0));
  return true;
}

// --sites FILE: allele_name<TAB>pos (1-based) per line; '#' lines and blank lines are skipped, a name that is not selected is counted and
// skipped; a malformed line or a pos outside its allele is an error that names the file and the line
static bool analyzerReadSites(t1k_job *job, const std::string &path, AnalyzerSitepile &sp) {
  const RefSet &R = job->ref;
  std::unordered_map<std::string, uint32_t> alleleOf;
  for (size_t a = 0; a < R.al.size(); ++a) alleleOf.emplace(R.al[a].name, (uint32_t)a);
  FILE *fp = fopen(path.c_str(), "r");
  if (!fp) { fprintf(stderr, "analyzer: cannot open %s\n", path.c_str()); return false; }
  std::string line;
  char buf[4096];
  uint64_t lineNo = 0;
  bool ok = true, more = true;
  while (ok && more) {
    line.clear();
    more = false;
    while (fgets(buf, sizeof buf, fp)) {
      more = true;
      line += buf;
      if (!line.empty() && line.back() == '\n') break;
    }
    if (!more) break;
    ++lineNo;
    while (!line.empty() && (line.back() == '\n' || line.back() == '\r')) line.pop_back();
    if (line.empty() || line[0] == '#') continue;
    const size_t tab = line.find('\t');
    char *end = nullptr;
    const long long pos = tab == std::string::npos ? 0 : strtoll(line.c_str() + tab + 1, &end, 10);
    if (tab == std::string::npos || tab == 0 || end == line.c_str() + tab + 1 || *end || !isdigit((unsigned char)line[tab + 1])) {
      fprintf(stderr, "analyzer: %s line %llu: expected allele_name<TAB>pos\n", path.c_str(), (unsigned long long)lineNo);
      ok = false;
      break;
    }
    auto it = alleleOf.find(line.substr(0, tab));
    if (it == alleleOf.end()) { ++sp.fileSkipped; continue; }
    if (pos < 1 || (unsigned long long)pos > R.seqs[it->second].size()) {
      fprintf(stderr, "analyzer: %s line %llu: pos %lld lies outside 1 .. %zu of %s\n", path.c_str(), (unsigned long long)lineNo, pos, R.seqs[it->second].size(), line.substr(0, tab).c_str());
      ok = false;
      break;
    }
    sp.fileSites.emplace_back(it->second, (uint32_t)(pos - 1));
  }
  fclose(fp);
  if (ok) fprintf(stderr, "--sites: %zu sites read from %s, %llu lines name an allele that is not selected\n", sp.fileSites.size(), path.c_str(), (unsigned long long)sp.fileSkipped);
  return ok;
}

// the sites of --barcodePileup, --phase and --siteSupport: the rows of _allele.vcf united with those of --sites, sorted and free of
// duplicates; per site the called bases in VCF order and the columns both files print for it
struct AnalyzerSiteList {
  std::vector<std::pair<uint32_t, uint32_t>> sites;
  std::map<std::pair<uint32_t, uint32_t>, std::string> varOf;
  std::vector<uint32_t> siteAllele, sitePos;
  std::vector<uint64_t> refOff;
  std::vector<int> exonPos;   // exonic position (SeqSet::GetExonicPosition), 0 = not exonic

  AnalyzerSiteList(t1k_job *job, const AnalyzerVariants &V, const AnalyzerSitepile &sp);
};

AnalyzerSiteList::AnalyzerSiteList(t1k_job *job, const AnalyzerVariants &V, const AnalyzerSitepile &sp) : sites(sp.fileSites) {
  const RefSet &R = job->ref;
  const size_t A = R.seqs.size();
  if (V.vc)
    for (const VariantRec &v : V.vc->variants) {
      const std::pair<uint32_t, uint32_t> k((uint32_t)v.allele, (uint32_t)v.refPos);
      sites.push_back(k);
      std::string &s = varOf[k];
      if (!s.empty()) s += ',';
      s += v.var;
    }
  std::sort(sites.begin(), sites.end());
  sites.erase(std::unique(sites.begin(), sites.end()), sites.end());
  const size_t nSites = sites.size();
  siteAllele.resize(nSites); sitePos.resize(nSites);
  for (size_t i = 0; i < nSites; ++i) { siteAllele[i] = sites[i].first; sitePos[i] = sites[i].second; }
  refOff.assign(A + 1, 0);
  for (size_t a = 0; a < A; ++a) refOff[a + 1] = refOff[a] + R.seqs[a].size();
  exonPos.assign(nSites, 0);  // one pass per allele
  for (size_t i = 0; i < nSites;) {
    const uint32_t a = siteAllele[i];
    int exonic = 0;
    uint32_t p = 0;
    for (; i < nSites && siteAllele[i] == a; ++i) {
      for (; p <= sitePos[i]; ++p) exonic += R.exon[a][p] ? 1 : 0;
      exonPos[i] = R.exon[a][sitePos[i]] ? exonic : 0;
    }
  }
}

// the replay session of the four sparse-table stages, behind the stage's _begin (rcBegin: what it returned): every kept piece
// through add(piece, &ms), the stage's _add; then its two-call _get, stats() and its _end.  keys / counts: the table's runs; msKernels, nRecs:
// summed over the pieces.  A failure is the job's (jobFail) and closes the session if it was open
static bool analyzerReplay(t1k_job *job, int rcBegin, const AnalyzerSitepile &sp, const std::function<int(const AnalyzerSitepile::Piece &, double *)> &add,
                           int (*get)(t1k_ctx *, uint64_t *, int32_t *, uint64_t, uint64_t *), const std::function<int()> &stats, int (*end)(t1k_ctx *), std::vector<uint64_t> &keys,
                           std::vector<int32_t> &counts, double &msKernels, uint64_t &nRecs) {
  t1k_ctx *ctx = job->ctx;
  auto fail = [&](int rc) { jobFail(job, rc, std::string("analyzer: ") + t1k_last_error(ctx)); fprintf(stderr, "analyzer: %s\n", t1k_job_last_error(job)); return false; };
  int rc = rcBegin;
  if (rc != T1K_OK) return fail(rc);
  for (const AnalyzerSitepile::Piece &pc : sp.pieces) {
    double ms = 0;
    if ((rc = add(pc, &ms)) != T1K_OK) {
      fail(rc);
      end(ctx);
      return false;
    }
    msKernels += ms;
    nRecs += pc.recs.size();
  }
  uint64_t nRuns = 0;
  if ((rc = get(ctx, nullptr, nullptr, 0, &nRuns)) == T1K_OK && nRuns) {
    keys.resize(nRuns); counts.resize(nRuns);
    rc = get(ctx, keys.data(), counts.data(), nRuns, &nRuns);
  }
  if (rc == T1K_OK) rc = stats();
  if (rc != T1K_OK) { fail(rc); end(ctx); return false; }
  if ((rc = end(ctx)) != T1K_OK) return fail(rc);
  return true;
}

// <prefix>_barcode_pileup.tsv: the kept pieces through t1k_sitepile_add at the sites, the runs that come back merged per (barcode, site)
// and written in barcode id order (the order of the lines of _barcode_expr.tsv), then allele, then pos
static bool analyzerSitepile(t1k_job *job, const std::string &prefix, const AnalyzerVariants &V, const AnalyzerSitepile &sp, const AnalyzerSiteList &L,
                             const std::vector<std::string> &barcodeNames) {
  const double t0 = nowMs();
  const RefSet &R = job->ref;
  const size_t A = R.seqs.size(), nSites = L.sites.size();
  const std::vector<uint32_t> &siteAllele = L.siteAllele, &sitePos = L.sitePos;
  const std::vector<uint64_t> &refOff = L.refOff;
  const std::vector<int> &exonPos = L.exonPos;
  t1k_ctx *ctx = job->ctx;
  double msKernels = 0, msFold = 0;
  uint64_t nRecs = 0, emitted = 0, folds = 0;
  std::vector<uint64_t> keys;
  std::vector<int32_t> counts;
  if (nSites && !analyzerReplay(job, t1k_sitepile_begin(ctx, (uint32_t)A, refOff.data(), nSites, siteAllele.data(), sitePos.data(), barcodeNames.size()), sp,
        [&](const AnalyzerSitepile::Piece &pc, double *ms) {
          return t1k_sitepile_add(ctx, pc.recs.data(), (uint32_t)pc.recs.size(), pc.bookPtr.data(), pc.book.data(), pc.pat.data(), pc.pat.size(), V.ops.data() + pc.ops0, pc.ops1 - pc.ops0, ms);
        }, t1k_sitepile_get, [&] { return t1k_sitepile_stats(ctx, &emitted, &folds, &msFold); }, t1k_sitepile_end, keys, counts, msKernels, nRecs)) return false;
  const double tw = nowMs();
  FILE *fp = fopen((prefix + "_barcode_pileup.tsv").c_str(), "w");
  if (!fp) { fprintf(stderr, "analyzer: cannot write %s_barcode_pileup.tsv\n", prefix.c_str()); return false; }
  fputs(kBarcodePileupHeader, fp);
  std::string out;
  char num[48];
  uint64_t cells = 0;
  for (size_t i = 0; i < keys.size();) {
    const uint64_t cell = keys[i] / 14;  // barcode * nSites + site: its runs are consecutive
    int32_t c[14] = {0};
    for (; i < keys.size() && keys[i] / 14 == cell; ++i) {
      const uint32_t plane = (uint32_t)((keys[i] % 14) >> 1);
      c[plane] += counts[i];                                  // a uniq booking counts in the plain counter as well
      if ((keys[i] & 1) == 0) c[7 + plane] += counts[i];
    }
    const uint64_t bc = cell / nSites, site = cell % nSites;
    const uint32_t a = siteAllele[site], pos = sitePos[site];
    ++cells;
    out += barcodeNames[bc];
    out += '\t';
    out += R.al[a].name;
    snprintf(num, sizeof num, "\t%u\t", pos + 1);
    out += num;
    if (exonPos[site]) { snprintf(num, sizeof num, "%d", exonPos[site]); out += num; } else out += '.';
    out += '\t';
    out += R.seqs[a][pos];
    out += '\t';
    auto it = L.varOf.find(L.sites[site]);
    out += it == L.varOf.end() ? std::string(".") : it->second;
    for (int k = 0; k < 14; ++k) { snprintf(num, sizeof num, "\t%d", c[k]); out += num; }
    out += '\n';
    if (out.size() >= (1u << 20)) { fwrite(out.data(), 1, out.size(), fp); out.clear(); }
  }
  fwrite(out.data(), 1, out.size(), fp);
  fclose(fp);
  if (getenv("T1K_DEBUG_PHASES"))
    fprintf(stderr, "barcode pileup: %zu sites, %llu records, %llu keys emitted, %llu folds, %llu cells; upload %.1f ms, kernels %.1f ms, fold %.1f ms, write %.1f ms\n", nSites,
            (unsigned long long)nRecs, (unsigned long long)emitted, (unsigned long long)folds, (unsigned long long)cells, std::max(0.0, (tw - t0) - msKernels - msFold), msKernels, msFold,
            nowMs() - tw);
  return true;
}

// <prefix>_allele_phase.tsv: the kept pieces through t1k_phase_add at the sites; one line per (site pair, state pair) with a
// booking, in key order: the alleles of job->ref.al, then pos1, pos2, obs1, obs2 in state order
static bool analyzerPhase(t1k_job *job, const std::string &prefix, const AnalyzerVariants &V, const AnalyzerSitepile &sp, const AnalyzerSiteList &L) {
  const double t0 = nowMs();
  const RefSet &R = job->ref;
  const size_t A = R.seqs.size(), nSites = L.sites.size();
  t1k_ctx *ctx = job->ctx;
  double msKernels = 0, msFold = 0;
  uint64_t nRecs = 0, nBook = 0, nObs = 0, nPaired = 0, emitted = 0, discordant = 0, folds = 0;
  std::vector<uint64_t> keys;
  std::vector<int32_t> counts;
  if (nSites && !analyzerReplay(job, t1k_phase_begin(ctx, (uint32_t)A, L.refOff.data(), nSites, L.siteAllele.data(), L.sitePos.data()), sp,
        [&](const AnalyzerSitepile::Piece &pc, double *ms) {
          nBook += pc.asgUniq.size();
          return t1k_phase_add(ctx, pc.recs.data(), (uint32_t)pc.recs.size(), (uint32_t)pc.asgUniq.size(), pc.asgRec.data(), pc.asgUniq.data(), pc.pat.data(), pc.pat.size(),
                               V.ops.data() + pc.ops0, pc.ops1 - pc.ops0, ms);
        }, t1k_phase_get, [&] { return t1k_phase_stats(ctx, &nObs, &nPaired, &emitted, &discordant, &folds, &msFold); }, t1k_phase_end, keys, counts, msKernels, nRecs)) return false;
  const double tw = nowMs();
  FILE *fp = fopen((prefix + "_allele_phase.tsv").c_str(), "w");
  if (!fp) { fprintf(stderr, "analyzer: cannot write %s_allele_phase.tsv\n", prefix.c_str()); return false; }
  fputs(kPhaseHeader, fp);
  static const char *kObs[6] = {"A", "C", "G", "T", "N", "-"};
  std::string out;
  uint64_t cells = 0;
  for (size_t i = 0; i < keys.size();) {
    const uint64_t cell = keys[i] >> 1;  // its uniq (even) run, then the other
    int32_t all = 0, uniq = 0;
    for (; i < keys.size() && (keys[i] >> 1) == cell; ++i) {
      all += counts[i];                                       // a uniq booking counts in the plain counter as well
      if ((keys[i] & 1) == 0) uniq += counts[i];
    }
    const uint64_t pair = cell / 36, s1 = pair / nSites, s2 = pair % nSites;
    const uint32_t a = L.siteAllele[s1];
    ++cells;
    out += R.al[a].name;
    for (uint64_t s : {s1, s2}) { out += '\t'; out += std::to_string(L.sitePos[s] + 1); }
    for (uint64_t s : {s1, s2}) { out += '\t'; out += L.exonPos[s] ? std::to_string(L.exonPos[s]) : std::string("."); }
    for (uint64_t s : {s1, s2}) { out += '\t'; out += R.seqs[a][L.sitePos[s]]; }
    for (uint64_t s : {s1, s2}) {
      auto it = L.varOf.find(L.sites[s]);
      out += '\t';
      out += it == L.varOf.end() ? std::string(".") : it->second;
    }
    out += '\t'; out += kObs[(cell % 36) / 6];
    out += '\t'; out += kObs[cell % 6];
    out += '\t' + std::to_string(all) + '\t' + std::to_string(uniq) + '\n';
    if (out.size() >= (1u << 20)) { fwrite(out.data(), 1, out.size(), fp); out.clear(); }
  }
  fwrite(out.data(), 1, out.size(), fp);
  fclose(fp);
  if (getenv("T1K_DEBUG_PHASES"))
    fprintf(stderr, "phase: %zu sites, %llu records, %llu bookings (%llu with two observed sites or more), %llu observations, %llu discordant, %llu keys emitted, %llu folds, %llu cells; "
                    "upload %.1f ms, kernels %.1f ms, fold %.1f ms, write %.1f ms\n", nSites, (unsigned long long)nRecs, (unsigned long long)nBook, (unsigned long long)nPaired,
            (unsigned long long)nObs, (unsigned long long)discordant, (unsigned long long)emitted, (unsigned long long)folds, (unsigned long long)cells,
            std::max(0.0, (tw - t0) - msKernels - msFold), msKernels, msFold, nowMs() - tw);
  return true;
}

// <prefix>_allele_support.tsv: the kept pieces through t1k_support_add at the sites; one line per (site, obs) with a booking,
// in key order: the alleles of job->ref.al, then pos, then obs in state order.  The runs come back as two families: family A (below 2^57)
// holds per (site, state, strand, mate, d, uniq) the bookings, family B per (site, state, orient, dStart, dEnd) one run per distinct
// template; both ascend by (site, state), so one pass over each folds them into lines.  nearEnd: bookings with d < nearEnd count as near_end
static bool analyzerSupport(t1k_job *job, const std::string &prefix, const AnalyzerVariants &V, const AnalyzerSitepile &sp, const AnalyzerSiteList &L, int nearEnd) {
  const double t0 = nowMs();
  const RefSet &R = job->ref;
  const size_t A = R.seqs.size(), nSites = L.sites.size();
  t1k_ctx *ctx = job->ctx;
  double msKernels = 0, msFold = 0;
  uint64_t nRecs = 0, nBook = 0, emitted = 0, folds = 0;
  std::vector<uint64_t> keys;
  std::vector<int32_t> counts;
  if (nSites && !analyzerReplay(job, t1k_support_begin(ctx, (uint32_t)A, L.refOff.data(), nSites, L.siteAllele.data(), L.sitePos.data()), sp,
        [&](const AnalyzerSitepile::Piece &pc, double *ms) {
          nBook += pc.supBook.size();
          return t1k_support_add(ctx, pc.recs.data(), (uint32_t)pc.recs.size(), pc.supRec.data(), pc.supBookPtr.data(), pc.supBook.data(), pc.pat.data(), pc.pat.size(),
                                 V.ops.data() + pc.ops0, pc.ops1 - pc.ops0, ms);
        }, t1k_support_get, [&] { return t1k_support_stats(ctx, &emitted, &folds, &msFold); }, t1k_support_end, keys, counts, msKernels, nRecs)) return false;
  const uint64_t nRuns = keys.size();
  const double tw = nowMs();
  FILE *fp = fopen((prefix + "_allele_support.tsv").c_str(), "w");
  if (!fp) { fprintf(stderr, "analyzer: cannot write %s_allele_support.tsv\n", prefix.c_str()); return false; }
  fputs(kSupportHeader, fp);
  static const char *kObs[7] = {"A", "C", "G", "T", "N", "-", "+"};
  const uint64_t familyB = 1ull << 57;
  const size_t nA = std::lower_bound(keys.begin(), keys.end(), familyB) - keys.begin();
  std::string out;
  char num[160];
  uint64_t lines = 0;
  size_t b = nA;
  std::vector<int64_t> hist(512);
  for (size_t i = 0; i < nA;) {
    const uint64_t cell = keys[i] >> 12;  // site * 7 + state: its family-A runs are consecutive
    int64_t all = 0, uniq = 0, strand[2] = {0, 0}, mate[2] = {0, 0};
    std::fill(hist.begin(), hist.end(), 0);
    for (; i < nA && (keys[i] >> 12) == cell; ++i) {
      const int64_t c = counts[i];
      all += c;                                               // a uniq booking counts in the plain counter as well
      if ((keys[i] & 1) == 0) uniq += c;
      strand[(keys[i] >> 11) & 1] += c;
      mate[(keys[i] >> 10) & 1] += c;
      hist[(keys[i] >> 1) & 511] += c;
    }
    int64_t templates = 0;                                    // its family-B runs: one per distinct template
    for (; b < keys.size() && ((keys[b] ^ familyB) >> 25) < cell; ++b) {}
    for (; b < keys.size() && ((keys[b] ^ familyB) >> 25) == cell; ++b) ++templates;
    int endMin = -1, endMed = -1;
    int64_t cum = 0, near = 0;
    for (int d = 0; d < 512; ++d) {
      if (!hist[d]) continue;
      if (endMin < 0) endMin = d;
      if (d < nearEnd) near += hist[d];
      cum += hist[d];
      if (endMed < 0 && 2 * cum >= all) endMed = d;           // the lower median: the first d whose cumulative count reaches ceil(all / 2)
    }
    const uint64_t site = cell / 7;
    const uint32_t a = L.siteAllele[site], pos = L.sitePos[site];
    ++lines;
    out += R.al[a].name;
    snprintf(num, sizeof num, "\t%u\t", pos + 1);
    out += num;
    out += L.exonPos[site] ? std::to_string(L.exonPos[site]) : std::string(".");
    out += '\t';
    out += R.seqs[a][pos];
    out += '\t';
    auto it = L.varOf.find(L.sites[site]);
    out += it == L.varOf.end() ? std::string(".") : it->second;
    out += '\t';
    out += kObs[cell % 7];
    snprintf(num, sizeof num, "\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%d\t%d\t%lld\t%lld\n", (long long)all, (long long)uniq, (long long)strand[0], (long long)strand[1], (long long)mate[0],
             (long long)mate[1], endMin, endMed, (long long)near, (long long)templates);
    out += num;
    if (out.size() >= (1u << 20)) { fwrite(out.data(), 1, out.size(), fp); out.clear(); }
  }
  fwrite(out.data(), 1, out.size(), fp);
  fclose(fp);
  if (getenv("T1K_DEBUG_PHASES"))
    fprintf(stderr, "site support: %zu sites, %llu records, %llu bookings, %llu keys emitted, %llu folds, %llu runs, %llu lines; upload %.1f ms, kernels %.1f ms, fold %.1f ms, write %.1f ms\n",
            nSites, (unsigned long long)nRecs, (unsigned long long)nBook, (unsigned long long)emitted, (unsigned long long)folds, (unsigned long long)nRuns, (unsigned long long)lines,
            std::max(0.0, (tw - t0) - msKernels - msFold), msKernels, msFold, nowMs() - tw);
  return true;
}

// <prefix>_allele_indel.tsv: the kept pieces through t1k_indel_add; the runs that come back ascend by (allele position after
// normalisation, type, payload, strand, uniq), so the four keys of an event are consecutive.  One line per event with at least minCount
// bookings, ordered by allele (job->ref.al order), pos, DEL before INS, len, seq.  job == NULL: the header alone
static bool analyzerIndels(t1k_job *job, const std::string &prefix, const AnalyzerVariants *V, const AnalyzerSitepile *sp, long minCount) {
  const double t0 = nowMs();
  struct Line { uint32_t allele, pos, ins, len; std::string seq; int64_t all, uniq, strand[2]; };
  std::vector<Line> lines;
  double msKernels = 0, msFold = 0;
  uint64_t nRecs = 0, nRuns = 0, events = 0, shifted = 0, edgeDel = 0, edgeIns = 0, emitted = 0, folds = 0;
  std::vector<uint64_t> refOff;
  if (job) {
    const RefSet &R = job->ref;
    const size_t A = R.seqs.size();
    t1k_ctx *ctx = job->ctx;
    // the alleles' bases back to back, reduced to A C G T N
    refOff.assign(A + 1, 0);
    for (size_t a = 0; a < A; ++a) refOff[a + 1] = refOff[a] + R.seqs[a].size();
    std::string refText;
    refText.reserve(refOff.back());
    for (const std::string &sq : R.seqs)
      for (char c : sq) { const char u = (char)toupper((unsigned char)c); refText += (u == 'A' || u == 'C' || u == 'G' || u == 'T') ? u : 'N'; }
    std::vector<uint64_t> keys;
    std::vector<int32_t> counts;
    if (!analyzerReplay(job, t1k_indel_begin(ctx, (uint32_t)A, refOff.data(), refText.data()), *sp,
          [&](const AnalyzerSitepile::Piece &pc, double *ms) {
            return t1k_indel_add(ctx, pc.recs.data(), (uint32_t)pc.recs.size(), pc.indStrand.data(), pc.indBookPtr.data(), pc.indBookUniq.data(), pc.pat.data(), pc.pat.size(),
                                 V->ops.data() + pc.ops0, pc.ops1 - pc.ops0, ms);
          }, t1k_indel_get, [&] { return t1k_indel_stats(ctx, &events, &shifted, &edgeDel, &edgeIns, &emitted, &folds, &msFold); }, t1k_indel_end, keys, counts, msKernels, nRecs)) return false;
    nRuns = keys.size();
    for (size_t i = 0; i < keys.size();) {
      const uint64_t ev = keys[i] >> 2;  // (g, type, payload): its runs are consecutive
      Line l{};
      for (; i < keys.size() && (keys[i] >> 2) == ev; ++i) {
        const int64_t c = counts[i];
        l.all += c;                                               // a uniq booking counts in the plain counter as well
        if ((keys[i] & 1) == 0) l.uniq += c;
        l.strand[(keys[i] >> 1) & 1] += c;
      }
      if (l.all < minCount) continue;
      const uint64_t g = ev >> 29;
      const uint32_t type = (uint32_t)(ev >> 27) & 3u, payload = (uint32_t)ev & ((1u << 27) - 1u);
      l.allele = (uint32_t)(std::upper_bound(refOff.begin(), refOff.end(), g) - refOff.begin() - 1);
      const uint32_t p = (uint32_t)(g - refOff[l.allele]);
      l.ins = type ? 1 : 0;
      l.pos = type ? p : p + 1;                                   // DEL: the first deleted base; INS: the base behind which it is inserted, 0 = in front of the first
      if (type == 0) { l.len = payload; l.seq = R.seqs[l.allele].substr(p, payload); }
      else if (type == 1) {
        for (l.len = 0; (payload >> (2 * l.len)) != 1u; ++l.len) {}
        for (uint32_t k = 0; k < l.len; ++k) l.seq += "ACGT"[(payload >> (2 * (l.len - 1 - k))) & 3u];
      } else { l.len = payload; l.seq = "*"; }
      lines.push_back(std::move(l));
    }
    std::sort(lines.begin(), lines.end(), [](const Line &x, const Line &y) { return std::tie(x.allele, x.pos, x.ins, x.len, x.seq) < std::tie(y.allele, y.pos, y.ins, y.len, y.seq); });
  }
  const double tw = nowMs();
  FILE *fp = fopen((prefix + "_allele_indel.tsv").c_str(), "w");
  if (!fp) { fprintf(stderr, "analyzer: cannot write %s_allele_indel.tsv\n", prefix.c_str()); return false; }
  fputs(kIndelHeader, fp);
  std::string out;
  char num[160];
  std::vector<int> exonic;  // of the allele being written: exonic bases up to and including each position
  for (size_t i = 0; i < lines.size(); ++i) {
    const Line &l = lines[i];
    const RefSet &R = job->ref;
    if (i == 0 || lines[i - 1].allele != l.allele) {
      const std::vector<uint8_t> &mask = R.exon[l.allele];
      exonic.resize(mask.size());
      int n = 0;
      for (size_t p = 0; p < mask.size(); ++p) exonic[p] = (n += mask[p] ? 1 : 0);
    }
    out += R.al[l.allele].name;
    snprintf(num, sizeof num, "\t%u\t", l.pos);
    out += num;
    if (l.pos >= 1 && R.exon[l.allele][l.pos - 1]) out += std::to_string(exonic[l.pos - 1]); else out += '.';
    snprintf(num, sizeof num, "\t%s\t%u\t", l.ins ? "INS" : "DEL", l.len);
    out += num;
    out += l.seq;
    snprintf(num, sizeof num, "\t%lld\t%lld\t%lld\t%lld\n", (long long)l.all, (long long)l.uniq, (long long)l.strand[0], (long long)l.strand[1]);
    out += num;
    if (out.size() >= (1u << 20)) { fwrite(out.data(), 1, out.size(), fp); out.clear(); }
  }
  fwrite(out.data(), 1, out.size(), fp);
  fclose(fp);
  if (job && getenv("T1K_DEBUG_PHASES"))
    fprintf(stderr, "indels: %llu records, %llu events, %llu shifted, %llu + %llu edge columns, %llu keys emitted, %llu folds, %llu runs, %zu lines; upload %.1f ms, kernels %.1f ms, fold %.1f ms, write %.1f ms\n",
            (unsigned long long)nRecs, (unsigned long long)events, (unsigned long long)shifted, (unsigned long long)edgeDel, (unsigned long long)edgeIns, (unsigned long long)emitted,
            (unsigned long long)folds, (unsigned long long)nRuns, lines.size(), std::max(0.0, (tw - t0) - msKernels - msFold), msKernels, msFold, nowMs() - tw);
  return true;
}

// --barcodeEM and --umi (§11.2): the lists BarcodeSummary counts.  The summary loop hands every counted fragment's kept
// list over in file order (bc = its row of the per-barcode table) and, under --umi, its UMI word.  runEM() groups the lists per barcode
// (identical sorted lists, first appearance first, host threads over barcodes) and runs t1k_barcode_em; --umi sends the same lists
// through t1k_umi_collapse and, with --barcodeEM, the molecules that come back through runEM() once more.
struct BarcodeLists {
  std::vector<uint32_t> fragRow;      // counted fragment -> its barcode id (the summary loop), then its row of the table
  std::vector<uint64_t> fragAt{0};    // counted fragment -> its sorted list in `lists`
  std::vector<uint32_t> lists;
  std::vector<uint64_t> fragUmi;      // --umi: counted fragment -> its UMI word (t1k_umi_collapse)
  std::vector<uint32_t> scratch;

  bool add(int bc, const uint32_t *alleles, uint32_t k) {
    scratch.assign(alleles, alleles + k);
    std::sort(scratch.begin(), scratch.end());
    scratch.erase(std::unique(scratch.begin(), scratch.end()), scratch.end());
    if (scratch.empty()) return false;  // nothing kept: not counted
    fragRow.push_back((uint32_t)bc);
    lists.insert(lists.end(), scratch.begin(), scratch.end());
    fragAt.push_back(lists.size());
    return true;
  }

  // rows x A expected counts (row-major), through the device.  sortGroups: a row's groups in ascending lexicographic order of their lists
  // instead of first appearance (molecules come in no particular order)
  int runEM(t1k_job *job, uint32_t nRows, double alpha, std::vector<double> &out, bool sortGroups = false, const char *what = "barcode EM") {
    const double t0 = nowMs();
    const size_t A = job->ref.al.size();
    const size_t nF = fragRow.size();
    // counted fragments per row, in file order (a stable counting sort)
    std::vector<uint64_t> rowStart(nRows + 1, 0);
    for (uint32_t r : fragRow) ++rowStart[r + 1];
    for (uint32_t r = 0; r < nRows; ++r) rowStart[r + 1] += rowStart[r];
    std::vector<uint32_t> byRow(nF);
    {
      std::vector<uint64_t> fill(rowStart.begin(), rowStart.end() - 1);
      for (size_t i = 0; i < nF; ++i) byRow[fill[fragRow[i]]++] = (uint32_t)i;
    }
    // per row: groups (distinct lists, first appearance first), their counts, U_b and the lists as indices into it
    struct Row { std::vector<uint32_t> U, entryPtr{0}, entry; std::vector<double> count; };
    std::vector<Row> R(nRows);
    parallelRanges(nRows, hostThreads(job), [&](int, size_t lo, size_t hi) {
      std::vector<uint32_t> slots, firstOf;  // open addressing over the row's groups; firstOf[g] = the fragment that opened group g
      for (size_t r = lo; r < hi; ++r) {
        Row &w = R[r];
        const uint64_t b = rowStart[r], e = rowStart[r + 1];
        size_t cap = 16;
        slots.assign(cap, ~0u);
        firstOf.clear();
        auto listOf = [&](uint32_t i) { return std::make_pair(lists.data() + fragAt[i], (size_t)(fragAt[i + 1] - fragAt[i])); };
        auto hashOf = [&](uint32_t i) {
          auto l = listOf(i);
          uint64_t h = 0x9E3779B97F4A7C15ull ^ l.second;
          for (size_t j = 0; j < l.second; ++j) { h = (h ^ l.first[j]) * 0xD6E8FEB86659FD93ull; h ^= h >> 29; }
          return h;
        };
        for (uint64_t q = b; q < e; ++q) {
          const uint32_t i = byRow[q];
          const auto l = listOf(i);
          size_t s = (size_t)hashOf(i) & (cap - 1);
          for (;; s = (s + 1) & (cap - 1)) {
            if (slots[s] == ~0u) {
              slots[s] = (uint32_t)firstOf.size();
              firstOf.push_back(i);
              w.count.push_back(1.0);
              break;
            }
            const auto m = listOf(firstOf[slots[s]]);
            if (m.second == l.second && std::equal(l.first, l.first + l.second, m.first)) { w.count[slots[s]] += 1.0; break; }
          }
          if (firstOf.size() * 2 > cap) {  // grow
            cap *= 2;
            slots.assign(cap, ~0u);
            for (uint32_t g = 0; g < firstOf.size(); ++g) {
              size_t t = (size_t)hashOf(firstOf[g]) & (cap - 1);
              while (slots[t] != ~0u) t = (t + 1) & (cap - 1);
              slots[t] = g;
            }
          }
        }
        if (sortGroups) {
          std::vector<uint32_t> ord(firstOf.size());
          std::iota(ord.begin(), ord.end(), 0u);
          std::sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) {
            const auto a = listOf(firstOf[x]), b = listOf(firstOf[y]);
            return std::lexicographical_compare(a.first, a.first + a.second, b.first, b.first + b.second);
          });
          std::vector<uint32_t> fo(ord.size());
          std::vector<double> ct(ord.size());
          for (size_t g = 0; g < ord.size(); ++g) { fo[g] = firstOf[ord[g]]; ct[g] = w.count[ord[g]]; }
          firstOf.swap(fo);
          w.count.swap(ct);
        }
        for (uint32_t i : firstOf) { auto l = listOf(i); w.U.insert(w.U.end(), l.first, l.first + l.second); }
        std::sort(w.U.begin(), w.U.end());
        w.U.erase(std::unique(w.U.begin(), w.U.end()), w.U.end());
        for (uint32_t i : firstOf) {
          auto l = listOf(i);
          for (size_t j = 0; j < l.second; ++j) w.entry.push_back((uint32_t)(std::lower_bound(w.U.begin(), w.U.end(), l.first[j]) - w.U.begin()));
          w.entryPtr.push_back((uint32_t)w.entry.size());
        }
      }
    });
    std::vector<uint64_t> bcAllelePtr(nRows + 1, 0), bcGroupPtr(nRows + 1, 0), groupEntryPtr(1, 0);
    std::vector<uint32_t> bcAllele, entryLocal;
    std::vector<double> groupCount;
    for (uint32_t r = 0; r < nRows; ++r) {
      const Row &w = R[r];
      bcAllele.insert(bcAllele.end(), w.U.begin(), w.U.end());
      bcAllelePtr[r + 1] = bcAllele.size();
      for (size_t g = 0; g < w.count.size(); ++g) groupEntryPtr.push_back(entryLocal.size() + w.entryPtr[g + 1]);
      entryLocal.insert(entryLocal.end(), w.entry.begin(), w.entry.end());
      groupCount.insert(groupCount.end(), w.count.begin(), w.count.end());
      bcGroupPtr[r + 1] = groupCount.size();
    }
    R.clear();
    // the prior: the pooled EM's allele shares (uniform if it has nothing)
    std::vector<double> rho(A);
    double tot = 0;
    for (size_t a = 0; a < A; ++a) tot += job->ref.al[a].abundance;
    for (size_t a = 0; a < A; ++a) rho[a] = tot > 0 ? job->ref.al[a].abundance / tot : 1.0 / (double)A;
    const double t1 = nowMs();
    std::vector<double> n(bcAllele.size());
    std::vector<int32_t> iters(nRows);
    double kernelMs = 0;
    int rc = t1k_barcode_em(job->ctx, nRows, bcAllelePtr.data(), bcAllele.data(), bcGroupPtr.data(), groupCount.data(), groupEntryPtr.data(), entryLocal.data(),
                            rho.data(), (uint32_t)A, alpha, 1e-7, 1000, n.data(), iters.data(), &kernelMs);
    if (rc != T1K_OK) return jobFail(job, rc, std::string("analyzer: ") + t1k_last_error(job->ctx));
    const double t2 = nowMs();
    out.assign((size_t)nRows * A, 0.0);
    for (uint32_t r = 0; r < nRows; ++r)
      for (uint64_t i = bcAllelePtr[r]; i < bcAllelePtr[r + 1]; ++i) out[(size_t)r * A + bcAllele[i]] = n[i];
    if (getenv("T1K_DEBUG_PHASES")) {
      int32_t mx = 0;
      double sum = 0;
      for (int32_t v : iters) { mx = std::max(mx, v); sum += v; }
      fprintf(stderr, "[t1k analyzer] %s: groups built in %.1f ms, t1k_barcode_em %.1f ms (kernel %.1f ms); %u barcodes, %zu groups, %zu entries; iterations max %d mean %.1f\n",
              what, t1 - t0, t2 - t1, kernelMs, nRows, groupCount.size(), entryLocal.size(), mx, nRows ? sum / nRows : 0.0);
    }
    return T1K_OK;
  }
};

// --umi FILE: one record per candidate read, >name\nUMI as the extractors write it, read by the project's reader (names as the read
// loader normalises them).  The analyzer's fragments are a subset of the records in the same relative order: take() is one forward merge.
struct UmiFile {
  ReadInput in;
  size_t cursor = 0;

  bool open(const std::string &path, int threads, std::string &err) {
    if (!in.open({path}, {}, "", hostThreadsFor(threads), err)) return false;
    const ReadInput::Side &s = in.side[0];
    for (size_t i = 0; i < s.seqL.size(); ++i)
      if (s.seqL[i] > 16) {
        err = "--umi takes UMIs of up to 16 bases: record " + std::string(s.idP[i], s.idL[i]) + " of " + path + " has " + std::to_string(s.seqL[i]);
        return false;
      }
    return true;
  }
  // 2 bits per base, first base most significant, the length above bit 32; all ones for a record that is not 1 - 16 of ACGT (an N, the
  // extractors' missing_barcode)
  static uint64_t word(const char *p, uint32_t n) {
    if (n < 1 || n > 16) return ~0ull;
    uint64_t code = 0;
    for (uint32_t i = 0; i < n; ++i) {
      const char c = p[i];
      const int b = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1;
      if (b < 0) return ~0ull;
      code = (code << 2) | (uint64_t)b;
    }
    return code | ((uint64_t)n << 32);
  }
  bool take(const char *id, size_t idLen, uint64_t &w) {
    const ReadInput::Side &s = in.side[0];
    for (; cursor < s.seqL.size(); ++cursor)
      if (s.idL[cursor] == idLen && !memcmp(s.idP[cursor], id, idLen)) {
        w = word(s.seqP[cursor], s.seqL[cursor]);
        ++cursor;
        return true;
      }
    return false;
  }
};

struct UmiTables {
  std::vector<double> frac;
  std::vector<int32_t> uniq;
  BarcodeLists molecules;  // the molecules as lists of their rows, for runEM()
};

// the counted fragments through t1k_umi_collapse: the molecule tables of nRows x A
static int analyzerUmiCollapse(t1k_job *job, const BarcodeLists &L, uint32_t nRows, int mismatch, double msFile, double msMerge, UmiTables &T) {
  const double t0 = nowMs();
  const size_t A = job->ref.al.size(), nF = L.fragRow.size();
  std::vector<uint32_t> alleleGene(A);
  uint32_t nGenes = 0;
  for (size_t a = 0; a < A; ++a) {
    if (job->ref.al[a].gene < 0) return jobFail(job, T1K_ERR_INTERNAL, "analyzer: allele " + job->ref.al[a].name + " has no gene");
    alleleGene[a] = (uint32_t)job->ref.al[a].gene;
    nGenes = std::max(nGenes, alleleGene[a] + 1);
  }
  if (nF >= (1ull << 31)) return jobFail(job, T1K_ERR_CAPACITY, "analyzer: --umi takes up to 2^31 counted fragments");
  // upper bounds: molecules <= fragments, their list entries <= the fragments'
  std::vector<uint32_t> fragMol(nF), molRow(nF), molFrags(nF);
  uint32_t nMol = 0;
  BarcodeLists &M = T.molecules;
  M.fragAt.assign(nF + 1, 0);
  M.lists.resize(L.lists.size());
  T.frac.assign((size_t)nRows * A, 0.0);
  T.uniq.assign((size_t)nRows * A, 0);
  t1k_umi_stats st;
  const double t1 = nowMs();
  const int rc = t1k_umi_collapse(job->ctx, (uint32_t)nF, L.fragRow.data(), L.fragUmi.data(), L.fragAt.data(), L.lists.data(), nRows, alleleGene.data(), (uint32_t)A, nGenes, mismatch,
                                  fragMol.data(), &nMol, molRow.data(), molFrags.data(), M.fragAt.data(), M.lists.data(), T.frac.data(), T.uniq.data(), &st);
  if (rc != T1K_OK) return jobFail(job, rc, std::string("analyzer: ") + t1k_last_error(job->ctx));
  const double t2 = nowMs();
  M.fragAt.resize((size_t)nMol + 1);
  M.lists.resize(M.fragAt[nMol]);
  M.fragRow.assign(molRow.begin(), molRow.begin() + nMol);
  const double t3 = nowMs();
  if (getenv("T1K_DEBUG_PHASES"))
    fprintf(stderr, "umi: %zu fragments, %llu distinct keys, %llu corrected UMIs, %u molecules, %llu split keys, %llu fragments without a UMI; host %.1f ms (UMI file %.1f, name merge %.1f, hand-over %.1f), t1k_umi_collapse %.1f ms, kernels %.1f ms\n",
            nF, (unsigned long long)st.keys, (unsigned long long)st.corrected, nMol, (unsigned long long)st.split, (unsigned long long)st.no_umi,
            msFile + msMerge + (t1 - t0) + (t3 - t2), msFile, msMerge, (t1 - t0) + (t3 - t2), t2 - t1, st.kernel_ms);
  return T1K_OK;
}

// <prefix>_aligned.sam opened and its header written: @HD, one @SQ per selected allele in job->ref.al order (the order of
// <prefix>_allele_pileup.tsv), @PG.  job == NULL: no allele is selected, no @SQ line
static bool analyzerSamOpen(t1k_job *job, const std::string &prefix, AnalyzerSam &sam) {
  sam.path = prefix + "_aligned.sam";
  sam.fp = fopen(sam.path.c_str(), "w");
  if (!sam.fp) { fprintf(stderr, "analyzer: cannot write %s\n", sam.path.c_str()); return false; }
  fputs("@HD\tVN:1.6\tSO:unsorted\tGO:query\n", sam.fp);
  if (job)
    for (size_t a = 0; a < job->ref.seqs.size(); ++a) fprintf(sam.fp, "@SQ\tSN:%s\tLN:%zu\n", job->ref.al[a].name.c_str(), job->ref.seqs[a].size());
  fputs("@PG\tID:t1k-analyzer\tPN:analyzer\n", sam.fp);
  return true;
}

// closes the file; T1K_DEBUG_PHASES: what the SAM output took
static bool analyzerSamClose(AnalyzerSam &sam) {
  const double t0 = nowMs();
  const bool ok = fclose(sam.fp) == 0;
  sam.fp = nullptr;
  if (!ok) { fprintf(stderr, "analyzer: cannot write %s\n", sam.path.c_str()); return false; }
  if (getenv("T1K_DEBUG_PHASES"))
    fprintf(stderr, "sam: %llu alignments encoded, %llu lines written, %llu CIGAR bytes, %llu MD bytes; calls %.1f ms, kernels %.1f ms, format + write %.1f ms\n", (unsigned long long)sam.nAln,
            (unsigned long long)sam.nLines, (unsigned long long)sam.cigarBytes, (unsigned long long)sam.mdBytes, sam.msCalls, sam.msKernels, sam.msWrite + (nowMs() - t0));
  return true;
}

static const char *kAnalyzerUsage =
    "./analyzer [OPTIONS]:   (MI355X build of the T1K post-analysis stage: re-assignment, novel variants, per-barcode summary)\n"
    "Required:\n"
    "\t-f STRING: fasta file with the allele reference sequences\n"
    "\t-a STRING: selected alleles list file (prefix_allele.tsv)\n"
    "\t-u STRING: single-end read file, or\n"
    "\t-1 STRING -2 STRING: paired-end read files\n"
    "Optional:\n"
    "\t-t INT: host threads (default: 1)\n"
    "\t-o STRING: output prefix (default: t1k)\n"
    "\t-n INT: maximal number of alleles per read (default: 2000)\n"
    "\t-s FLOAT: minimum alignment similarity (default: 0.8)\n"
    "\t--barcode STRING: barcode file\n"
    "\t--barcodeEM: also write prefix_barcode_em.tsv, the alleles' expected fragment counts of an EM run per barcode (needs --barcode; or $T1K_BARCODE_EM=1 with --barcode)\n"
    "\t--barcodeEMPrior FLOAT: weight of the pooled allele abundances as a prior of the per-barcode EM (default: 0)\n"
    "\t--umi FILE: UMI file (prefix_umi.fa of bam-extractor --UMI): also write prefix_barcode_umi.tsv, the table of prefix_barcode_expr.tsv counted in molecules\n"
    "\t\tinstead of fragments, and with --barcodeEM prefix_barcode_umi_em.tsv (needs --barcode)\n"
    "\t--umiMismatch INT: 1 joins a UMI to a neighbour at one mismatch that is at least twice as frequent, 0 keeps every UMI (default: 1)\n"
    "\t--pileup: also write prefix_allele_pileup.tsv, per base of every selected allele the read bases, deletions and inserted bases of the alignments\n"
    "\t\tthe variant pass holds, over all assignments and over those of fragments with one assignment (_uniq)\n"
    "\t--barcodePileup: also write prefix_barcode_pileup.tsv, the counters of --pileup per barcode at the positions of prefix_allele.vcf and of --sites,\n"
    "\t\tone line per (barcode, site) with a read (needs --barcode)\n"
    "\t--phase: also write prefix_allele_phase.tsv, for every two of the positions of prefix_allele.vcf and of --sites on one allele the fragments that\n"
    "\t\tshow both, by what they show there (A C G T N or - for a deletion): read-backed phasing of the variants\n"
    "\t--sam: also write prefix_aligned.sam, the alignments the variant pass holds as SAM records on the selected alleles (CIGAR, NM, MD, NH, HI), one line per\n"
    "\t\taligned read-end of every assignment of every assigned fragment (no counterpart in the reference)\n"
    "\t--siteSupport: also write prefix_allele_support.tsv, for the positions of prefix_allele.vcf and of --sites one line per observed base, deletion (-) or\n"
    "\t\tinserted base (+): the bookings of --pileup there by strand, by mate, by distance from the read-end's nearer end, and the distinct templates behind them\n"
    "\t--supportEnd INT: bookings fewer than INT bases from an end of their read-end count in the near_end column of --siteSupport, 0 .. 511 (default: 10)\n"
    "\t--indels: also write prefix_allele_indel.tsv, the insertions and deletions inside the alignments the variant pass holds, one line per event and allele,\n"
    "\t\tleft-aligned against the allele: its bookings, those of fragments with one assignment, and the bookings by strand (no counterpart in the reference)\n"
    "\t--indelMinCount INT: print only the lines of --indels whose count reaches INT, 1 .. 2147483647 (default: 1)\n"
    "\t--sites FILE: more sites for --barcodePileup and --phase, and for --siteSupport, one per line as allele_name<TAB>pos (1-based, the pos column of prefix_allele_pileup.tsv); '#' lines,\n"
    "\t\tblank lines and alleles that are not selected are skipped\n"
    "\t--relaxIntronAlign: allow one more mismatch in intronic alignment\n"
    "\t--alleleDigitUnits INT, --alleleDelimiter CHR: as in genotyper\n"
    "\t--varMaxGroup INT: the maximum variant group size to call novel variant. -1 for no limitation, 0 for no variant calling (default: 8)\n"
    "\t--device INT: GPU ordinal (default: $T1K_DEVICE or 0)\n";

int t1k_analyzer_main(int argc, char **argv) {
  if (argc <= 1) { fprintf(stderr, "%s", kAnalyzerUsage); return 0; }  // Analyzer.cpp:241-245
  static struct option longOpts[] = {{"barcode", required_argument, 0, 10000}, {"relaxIntronAlign", no_argument, 0, 10004}, {"alleleDigitUnits", required_argument, 0, 10005},
                                     {"alleleDelimiter", required_argument, 0, 10006}, {"varMaxGroup", required_argument, 0, 10007}, {"device", required_argument, 0, 10010},
                                     {"barcodeEM", no_argument, 0, 10011}, {"barcodeEMPrior", required_argument, 0, 10012}, {"umi", required_argument, 0, 10013},
                                     {"umiMismatch", required_argument, 0, 10014}, {"pileup", no_argument, 0, 10015}, {"barcodePileup", no_argument, 0, 10016},
                                     {"sites", required_argument, 0, 10017}, {"phase", no_argument, 0, 10018}, {"sam", no_argument, 0, 10019},
                                     {"siteSupport", no_argument, 0, 10020}, {"supportEnd", required_argument, 0, 10021}, {"indels", no_argument, 0, 10022},
                                     {"indelMinCount", required_argument, 0, 10023}, {0, 0, 0, 0}};
  t1k_job_params p;
  t1k_job_params_default(&p);
  if (const char *d = getenv("T1K_DEVICE")) p.device = atoi(d);
  std::string refFile, alleleFile, prefix = "t1k", barcode;
  std::vector<const char *> f1, f2, single;
  int varMaxGroup = 8;  // Analyzer.cpp:251
  bool barcodeEM = false, pileup = false, barcodePileup = false, phase = false, samOut = false, siteSupport = false, indels = false;
  double emPrior = 0;
  const char *emPriorText = nullptr, *umiMismatchText = nullptr, *supportEndText = nullptr, *indelMinText = nullptr;
  int supportEnd = 10;
  long indelMinCount = 1;
  std::string umiPath, sitesPath;
  int umiMismatch = 1;
  optind = 1;
  int c, idx = 0;
  while ((c = getopt_long(argc, argv, "f:a:u:1:2:o:t:n:s:", longOpts, &idx)) != -1) {
    switch (c) {
      case 'f': refFile = optarg; break;
      case 'a': alleleFile = optarg; break;
      case 'u': single.push_back(optarg); break;
      case '1': f1.push_back(optarg); break;
      case '2': f2.push_back(optarg); break;
      case 'o': prefix = optarg; break;
      case 't': p.threads = atoi(optarg); break;
      case 'n': p.dev.max_assign_cnt = atoi(optarg); break;
      case 's': p.dev.ref_seq_similarity = atof(optarg); break;
      case 10000: barcode = optarg; break;
      case 10004: p.dev.relax_intron_align = 1; break;
      case 10005: p.allele_digit_units = atoi(optarg); break;
      case 10006: p.allele_delimiter = optarg[0]; break;
      case 10007: varMaxGroup = atoi(optarg); break;
      case 10010: p.device = atoi(optarg); break;
      case 10011: barcodeEM = true; break;
      case 10012: emPriorText = optarg; break;
      case 10013: umiPath = optarg; break;
      case 10014: umiMismatchText = optarg; break;
      case 10015: pileup = true; break;
      case 10016: barcodePileup = true; break;
      case 10017: sitesPath = optarg; break;
      case 10018: phase = true; break;
      case 10019: samOut = true; break;
      case 10020: siteSupport = true; break;
      case 10021: supportEndText = optarg; break;
      case 10022: indels = true; break;
      case 10023: indelMinText = optarg; break;
      default: fprintf(stderr, "%s", kAnalyzerUsage); return EXIT_FAILURE;
    }
  }
  if (refFile.empty()) { fprintf(stderr, "Need to use -f to specify the reference sequences.\n"); return EXIT_FAILURE; }
  if (alleleFile.empty()) { fprintf(stderr, "Need to use -a to specify selected allele ids.\n"); return EXIT_FAILURE; }
  if (barcodeEM && barcode.empty()) { fprintf(stderr, "--barcodeEM needs --barcode.\n"); return EXIT_FAILURE; }
  if (const char *e = getenv("T1K_BARCODE_EM"))  // (for run-t1k, which passes the analyzer only the flags it knows)
    if (!strcmp(e, "1") && !barcode.empty()) barcodeEM = true;
  if (emPriorText) {
    char *end = nullptr;
    emPrior = strtod(emPriorText, &end);
    if (end == emPriorText || *end || !(emPrior >= 0) || !std::isfinite(emPrior)) { fprintf(stderr, "--barcodeEMPrior needs a number >= 0.\n"); return EXIT_FAILURE; }
  }
  if (!umiPath.empty() && barcode.empty()) { fprintf(stderr, "--umi needs --barcode.\n"); return EXIT_FAILURE; }
  if (barcodePileup && barcode.empty()) { fprintf(stderr, "--barcodePileup needs --barcode.\n"); return EXIT_FAILURE; }
  if (!sitesPath.empty() && !barcodePileup && !phase && !siteSupport) { fprintf(stderr, "--sites has no meaning without --barcodePileup, --phase or --siteSupport: ignored.\n"); sitesPath.clear(); }
  if (supportEndText) {
    char *end = nullptr;
    const long v = strtol(supportEndText, &end, 10);
    if (end == supportEndText || *end || !isdigit((unsigned char)supportEndText[0]) || v < 0 || v > 511) { fprintf(stderr, "--supportEnd needs an integer from 0 to 511.\n"); return EXIT_FAILURE; }
    supportEnd = (int)v;
  }
  if (indelMinText && !indels) { fprintf(stderr, "--indelMinCount has no meaning without --indels: ignored.\n"); indelMinText = nullptr; }
  if (indelMinText) {
    char *end = nullptr;
    errno = 0;
    const long long v = strtoll(indelMinText, &end, 10);
    if (end == indelMinText || *end || !isdigit((unsigned char)indelMinText[0]) || errno || v < 1 || v > 2147483647ll) { fprintf(stderr, "--indelMinCount needs an integer from 1 to 2147483647.\n"); return EXIT_FAILURE; }
    indelMinCount = (long)v;
  }
  if (umiMismatchText) {
    if (strcmp(umiMismatchText, "0") && strcmp(umiMismatchText, "1")) { fprintf(stderr, "--umiMismatch needs 0 or 1.\n"); return EXIT_FAILURE; }
    umiMismatch = atoi(umiMismatchText);
  }
  const bool umi = !umiPath.empty();
  std::unique_ptr<UmiFile> umiFile;
  double msUmiHost = 0, msUmiMerge = 0;
  if (umi) {  // mapped and checked before anything else runs
    const double t0 = nowMs();
    std::string err;
    umiFile.reset(new UmiFile);
    if (!umiFile->open(umiPath, p.threads, err)) { fprintf(stderr, "analyzer: %s\n", err.c_str()); return EXIT_FAILURE; }
    msUmiHost += nowMs() - t0;
  }
  if (p.dev.max_assign_cnt == 0) p.dev.max_assign_cnt = -1;
  std::set<std::string> selected;
  {
    FILE *fp = fopen(alleleFile.c_str(), "r");  // first word of every line (Analyzer.cpp:347-356)
    if (!fp) { fprintf(stderr, "analyzer: cannot open %s\n", alleleFile.c_str()); return EXIT_FAILURE; }
    char line[10241], name[10241];
    while (fgets(line, sizeof(line), fp))
      if (sscanf(line, "%10240s", name) == 1) selected.insert(name);
    fclose(fp);
  }
  if (selected.empty()) {
    // nothing was genotyped (run-t1k starts the analyzer all the same): the reference loads no sequence, assigns no fragment and
    // leaves an empty VCF and a per-barcode table that is only its header
    FILE *fv = fopen((prefix + "_allele.vcf").c_str(), "w");
    if (!fv) { fprintf(stderr, "analyzer: cannot write %s_allele.vcf\n", prefix.c_str()); return EXIT_FAILURE; }
    fclose(fv);
    if (!barcode.empty()) {
      FILE *fb = fopen((prefix + "_barcode_expr.tsv").c_str(), "w");
      if (!fb) { fprintf(stderr, "analyzer: cannot write %s_barcode_expr.tsv\n", prefix.c_str()); return EXIT_FAILURE; }
      fprintf(fb, "#barcode\n");
      fclose(fb);
    }
    const std::pair<const char *, bool> extra[] = {{"_barcode_em.tsv", barcodeEM}, {"_barcode_umi.tsv", umi}, {"_barcode_umi_em.tsv", umi && barcodeEM}};
    for (const auto &x : extra) {
      if (!x.second) continue;
      const char *name = x.first;
      FILE *fe = fopen((prefix + name).c_str(), "w");
      if (!fe) { fprintf(stderr, "analyzer: cannot write %s%s\n", prefix.c_str(), name); return EXIT_FAILURE; }
      fprintf(fe, "#barcode\n");
      fclose(fe);
    }
    if (pileup && !analyzerWritePileup(nullptr, prefix, nullptr)) return EXIT_FAILURE;
    if (barcodePileup) {  // (no allele is selected: every name of --sites would be skipped)
      FILE *fs = fopen((prefix + "_barcode_pileup.tsv").c_str(), "w");
      if (!fs) { fprintf(stderr, "analyzer: cannot write %s_barcode_pileup.tsv\n", prefix.c_str()); return EXIT_FAILURE; }
      fputs(kBarcodePileupHeader, fs);
      fclose(fs);
    }
    if (phase) {
      FILE *fs = fopen((prefix + "_allele_phase.tsv").c_str(), "w");
      if (!fs) { fprintf(stderr, "analyzer: cannot write %s_allele_phase.tsv\n", prefix.c_str()); return EXIT_FAILURE; }
      fputs(kPhaseHeader, fs);
      fclose(fs);
    }
    if (siteSupport) {
      FILE *fs = fopen((prefix + "_allele_support.tsv").c_str(), "w");
      if (!fs) { fprintf(stderr, "analyzer: cannot write %s_allele_support.tsv\n", prefix.c_str()); return EXIT_FAILURE; }
      fputs(kSupportHeader, fs);
      fclose(fs);
    }
    if (indels && !analyzerIndels(nullptr, prefix, nullptr, nullptr, indelMinCount)) return EXIT_FAILURE;
    if (samOut) {
      AnalyzerSam sam;
      if (!analyzerSamOpen(nullptr, prefix, sam) || !analyzerSamClose(sam)) return EXIT_FAILURE;
    }
    logLine("Post analysis finishes.");
    return 0;
  }
  t1k_job *job = nullptr;
  int rc = jobCreate(&p, refFile.c_str(), &selected, &job);
  if (rc != T1K_OK) {
    fprintf(stderr, "analyzer: %s\n", job ? t1k_job_last_error(job) : "initialisation failed");
    t1k_job_destroy(job);
    return EXIT_FAILURE;
  }
  job->analyzer = true;
  std::unique_ptr<AnalyzerSitepile> sp(barcodePileup || phase || siteSupport || indels ? new AnalyzerSitepile : nullptr);
  if (sp) { sp->barcodes = barcodePileup; sp->phase = phase; sp->support = siteSupport; sp->indels = indels; }
  if (sp && !sitesPath.empty() && !analyzerReadSites(job, sitesPath, *sp)) { t1k_job_destroy(job); return EXIT_FAILURE; }
  const bool paired = !f2.empty();
  const std::vector<const char *> &first = !f1.empty() ? f1 : single;
  if (first.empty()) { fprintf(stderr, "analyzer: no read file given (-u, or -1 and -2)\n"); t1k_job_destroy(job); return EXIT_FAILURE; }
  rc = t1k_job_load_reads_multi(job, first.data(), (uint32_t)first.size(), paired ? f2.data() : nullptr, (uint32_t)f2.size(), barcode.empty() ? nullptr : barcode.c_str());
  if (rc != T1K_OK) { fprintf(stderr, "analyzer: %s\n", t1k_job_last_error(job)); t1k_job_destroy(job); return EXIT_FAILURE; }
  const ReadInput &in = *job->in;
  const uint32_t F = (uint32_t)in.nFrag();
  logLine("Found %d read fragments. Start read assignment.", (int)F);
  rc = t1k_job_run_local(job);
  if (rc != T1K_OK) { fprintf(stderr, "analyzer: %s\n", t1k_job_last_error(job)); t1k_job_destroy(job); return EXIT_FAILURE; }
  logLine("Finish read end assignments.");
  uint64_t nAssigned = 0;
  for (uint32_t f = 0; f < F; ++f) nAssigned += job->fragAssigned[f] ? 1 : 0;
  logLine("Finish read fragment assignments. %d read fragments can be assigned.", (int)nAssigned);
  // barcode ids in order of first appearance over ALL loaded fragments (Analyzer.cpp:380-392): the rows of the per-barcode tables, and the
  // barcodes of --barcodePileup's bookings, which the variant pass collects
  std::vector<std::string> names;
  std::vector<int> bcOf;
  if (in.hasBarcode) {
    std::unordered_map<std::string, int> idOf;
    bcOf.resize(F);
    for (uint32_t f = 0; f < F; ++f) {
      const uint32_t r = in.frag[f];
      std::string s(in.bc.seqP[r], in.bc.seqL[r]);
      auto it = idOf.find(s);
      if (it == idOf.end()) { it = idOf.emplace(s, (int)names.size()).first; names.push_back(s); }
      bcOf[f] = it->second;
    }
  }
  if (barcodePileup && !in.hasBarcode) { fprintf(stderr, "analyzer: --barcodePileup: the barcode file gave no barcodes\n"); t1k_job_destroy(job); return EXIT_FAILURE; }
  if (sp) sp->bcOf = &bcOf;
  AnalyzerVariants V;
  std::unique_ptr<AnalyzerPileup> pile(pileup ? new AnalyzerPileup : nullptr);
  std::unique_ptr<AnalyzerSam> sam(samOut ? new AnalyzerSam : nullptr);
  if (sam && !analyzerSamOpen(job, prefix, *sam)) { t1k_job_destroy(job); return EXIT_FAILURE; }
  if (varMaxGroup != 0) {  // (0: VariantCaller::ComputeVariant returns before it looks at a read, VariantCaller.hpp:980-981)
    rc = analyzerCallVariants(job, varMaxGroup, V, pile.get(), sp.get(), sam.get());
    if (rc != T1K_OK) { fprintf(stderr, "analyzer: %s\n", t1k_job_last_error(job)); t1k_job_destroy(job); return EXIT_FAILURE; }
    logLine("Finish allele quantification in %d EM iterations.", V.emIterations);
  } else if (pileup || sam || indels || (sp && !sp->fileSites.empty())) {
    // no variant is called, but the pileup is of the alignments of steps (1) - (3): they run, VariantCaller does not (V.vc stays empty: the
    // VCF is the empty file and the per-barcode table counts the raw lists).  --barcodePileup, --phase and --siteSupport without sites of their own have nothing to book.
    rc = analyzerAlignAssignments(job, V, pile.get(), sp.get(), sam.get());
    if (rc != T1K_OK) { fprintf(stderr, "analyzer: %s\n", t1k_job_last_error(job)); t1k_job_destroy(job); return EXIT_FAILURE; }
  } else if (barcodeEM && emPrior > 0) {
    // the per-barcode EM's prior is the pooled EM's abundances: step (1) of the variant pass on its own (its outputs are not written)
    std::vector<uint32_t> cnt;
    std::vector<uint64_t> rowAt;
    std::vector<t1k_row_entry> rows;
    int it = 0;
    rc = analyzerRows(job, cnt, rowAt, rows);
    if (rc == T1K_OK) rc = analyzerPooledEM(job, cnt, rowAt, rows, &it);
    if (rc != T1K_OK) { fprintf(stderr, "analyzer: %s\n", t1k_job_last_error(job)); t1k_job_destroy(job); return EXIT_FAILURE; }
  }
  if (sam) {
    if (!analyzerSamClose(*sam)) { t1k_job_destroy(job); return EXIT_FAILURE; }
    sam.reset();
  }
  {
    FILE *fp = fopen((prefix + "_allele.vcf").c_str(), "w");  // VariantCaller::OutputAlleleVCF (1202-1227)
    if (!fp) { fprintf(stderr, "analyzer: cannot write %s_allele.vcf\n", prefix.c_str()); t1k_job_destroy(job); return EXIT_FAILURE; }
    if (V.vc) { const std::string text = V.vc->vcfText(); fwrite(text.data(), 1, text.size(), fp); }
    fclose(fp);
  }
  if (pile) {
    if (!analyzerWritePileup(job, prefix, pile.get())) { t1k_job_destroy(job); return EXIT_FAILURE; }
    pile.reset();
  }
  if (sp) {
    const AnalyzerSiteList siteList(job, V, *sp);
    if (barcodePileup && !analyzerSitepile(job, prefix, V, *sp, siteList, names)) { t1k_job_destroy(job); return EXIT_FAILURE; }
    if (phase && !analyzerPhase(job, prefix, V, *sp, siteList)) { t1k_job_destroy(job); return EXIT_FAILURE; }
    if (siteSupport && !analyzerSupport(job, prefix, V, *sp, siteList, supportEnd)) { t1k_job_destroy(job); return EXIT_FAILURE; }
    if (indels && !analyzerIndels(job, prefix, &V, sp.get(), indelMinCount)) { t1k_job_destroy(job); return EXIT_FAILURE; }
    sp.reset();
  }
  if (in.hasBarcode) {
    // counts in fragment order
    const size_t A = job->ref.al.size();
    std::map<int, std::pair<std::vector<double>, std::vector<int>>> table;  // barcode -> (fractional counts, unique counts)
    const uint32_t step = 1u << 18;
    std::vector<uint32_t> cnt;
    std::vector<t1k_row_entry> rows;
    std::vector<uint8_t> keepFlag;
    std::unique_ptr<BarcodeLists> em(barcodeEM || umi ? new BarcodeLists : nullptr);
    std::vector<uint32_t> emList;
    std::vector<uint32_t> countedFrag;  // --umi: the counted fragments, for the name merge behind the loop
    for (uint32_t f0 = 0; f0 < F; f0 += step) {
      const uint32_t n = std::min(step, F - f0);
      cnt.resize(n);
      uint64_t total = 0;
      rc = t1k_rowset_rows_download(job->rows, f0, n, cnt.data(), nullptr, 0, &total);
      rows.resize(total);
      if (rc == T1K_OK && total) rc = t1k_rowset_rows_download(job->rows, f0, n, cnt.data(), rows.data(), total, &total);
      if (rc != T1K_OK) { fprintf(stderr, "analyzer: %s\n", t1k_rowset_last_error(job->rows)); t1k_job_destroy(job); return EXIT_FAILURE; }
      uint64_t q = 0;
      for (uint32_t i = 0; i < n; ++i) {
        const uint32_t k = cnt[i];
        if (!job->fragAssigned[f0 + i]) { q += k; continue; }
        auto &slot = table[bcOf[f0 + i]];  // BarcodeSummary::AddFragment (BarcodeSummary.hpp:24-57)
        if (slot.first.empty()) { slot.first.assign(A, 0.0); slot.second.assign(A, 0); }
        if (V.vc) {  // the assignments VariantCaller::AdjustFragmentAssignment keeps (1229-1311)
          const uint32_t f = f0 + i;
          VariantCaller::Fragment fr;
          fr.asg = V.asg.data() + V.asgPtr[f]; fr.n = (uint32_t)(V.asgPtr[f + 1] - V.asgPtr[f]);
          const uint32_t r = in.frag[f];
          fr.r1 = in.side[0].seqP[r]; fr.l1 = in.side[0].seqL[r];
          if (in.paired) { fr.r2 = in.side[1].seqP[r]; fr.l2 = in.side[1].seqL[r]; }
          keepFlag.assign(k, 0);
          if (fr.n == k) V.vc->adjust(fr, V.ops.data(), keepFlag.data());
          uint32_t kept = 0;
          for (uint32_t j = 0; j < k; ++j) kept += keepFlag[j];
          if (em) {
            emList.clear();
            for (uint32_t j = 0; j < k; ++j) if (keepFlag[j]) emList.push_back((uint32_t)rows[q + j].allele_idx);
            if (em->add(bcOf[f], emList.data(), (uint32_t)emList.size()) && umi) countedFrag.push_back(f);
          }
          for (uint32_t j = 0; j < k; ++j, ++q) {
            if (!keepFlag[j]) continue;
            slot.first[rows[q].allele_idx] += 1.0 / kept;
            if (kept == 1) ++slot.second[rows[q].allele_idx];
          }
          continue;
        }
        if (em) {
          emList.clear();
          for (uint32_t j = 0; j < k; ++j) emList.push_back((uint32_t)rows[q + j].allele_idx);
          if (em->add(bcOf[f0 + i], emList.data(), k) && umi) countedFrag.push_back(f0 + i);
        }
        for (uint32_t j = 0; j < k; ++j, ++q) {
          slot.first[rows[q].allele_idx] += 1.0 / k;
          if (k == 1) ++slot.second[rows[q].allele_idx];
        }
      }
    }
    if (umi) {
      // every counted fragment's UMI word: the record of the UMI file that carries its read's name, one forward merge
      const double t0 = nowMs();
      em->fragUmi.resize(countedFrag.size());
      for (size_t i = 0; i < countedFrag.size(); ++i) {
        const uint32_t r = in.frag[countedFrag[i]];
        if (in.noIds || !umiFile->take(in.side[0].idP[r], in.side[0].idL[r], em->fragUmi[i])) {
          fprintf(stderr, "analyzer: read %s has no record in %s (the UMI file lists the reads in the order of the read files)\n",
                  in.noIds ? "(unnamed)" : std::string(in.side[0].idP[r], in.side[0].idL[r]).c_str(), umiPath.c_str());
          t1k_job_destroy(job);
          return EXIT_FAILURE;
        }
      }
      msUmiMerge = nowMs() - t0;
    }
    FILE *fp = fopen((prefix + "_barcode_expr.tsv").c_str(), "w");  // BarcodeSummary::Output (59-80)
    if (!fp) { fprintf(stderr, "analyzer: cannot write %s_barcode_expr.tsv\n", prefix.c_str()); t1k_job_destroy(job); return EXIT_FAILURE; }
    fprintf(fp, "#barcode");
    for (size_t a = 0; a < A; ++a) fprintf(fp, "\t%s", job->ref.al[a].name.c_str());
    for (size_t a = 0; a < A; ++a) fprintf(fp, "\t%s_uniq", job->ref.al[a].name.c_str());
    fprintf(fp, "\n");
    for (auto &kv : table) {
      fprintf(fp, "%s", names[kv.first].c_str());
      for (size_t a = 0; a < A; ++a) fprintf(fp, "\t%lf", kv.second.first[a]);
      for (size_t a = 0; a < A; ++a) fprintf(fp, "\t%d", kv.second.second[a]);
      fprintf(fp, "\n");
    }
    fclose(fp);
    if (em) {
      // the table's rows, in its order: every counted fragment's barcode id becomes its row
      std::unordered_map<int, uint32_t> rowOf;
      for (auto &kv : table) rowOf.emplace(kv.first, (uint32_t)rowOf.size());
      for (uint32_t &r : em->fragRow) r = rowOf.at((int)r);
    }
    // <prefix><name>: a table of expected counts in the rows of _barcode_expr.tsv
    auto writeEstimates = [&](const char *name, const std::vector<double> &est) -> bool {
      FILE *fe = fopen((prefix + name).c_str(), "w");
      if (!fe) { fprintf(stderr, "analyzer: cannot write %s%s\n", prefix.c_str(), name); return false; }
      fprintf(fe, "#barcode");
      for (size_t a = 0; a < A; ++a) fprintf(fe, "\t%s", job->ref.al[a].name.c_str());
      fprintf(fe, "\n");
      size_t r = 0;
      for (auto &kv : table) {
        fprintf(fe, "%s", names[kv.first].c_str());
        for (size_t a = 0; a < A; ++a) fprintf(fe, "\t%lf", est[r * A + a]);
        fprintf(fe, "\n");
        ++r;
      }
      fclose(fe);
      return true;
    };
    if (barcodeEM) {
      std::vector<double> est;
      if (em->runEM(job, (uint32_t)table.size(), emPrior, est) != T1K_OK) { fprintf(stderr, "analyzer: %s\n", t1k_job_last_error(job)); t1k_job_destroy(job); return EXIT_FAILURE; }
      if (!writeEstimates("_barcode_em.tsv", est)) { t1k_job_destroy(job); return EXIT_FAILURE; }
    }
    if (umi) {
      UmiTables T;
      if (analyzerUmiCollapse(job, *em, (uint32_t)table.size(), umiMismatch, msUmiHost, msUmiMerge, T) != T1K_OK) { fprintf(stderr, "analyzer: %s\n", t1k_job_last_error(job)); t1k_job_destroy(job); return EXIT_FAILURE; }
      FILE *fu = fopen((prefix + "_barcode_umi.tsv").c_str(), "w");  // the layout of _barcode_expr.tsv
      if (!fu) { fprintf(stderr, "analyzer: cannot write %s_barcode_umi.tsv\n", prefix.c_str()); t1k_job_destroy(job); return EXIT_FAILURE; }
      fprintf(fu, "#barcode");
      for (size_t a = 0; a < A; ++a) fprintf(fu, "\t%s", job->ref.al[a].name.c_str());
      for (size_t a = 0; a < A; ++a) fprintf(fu, "\t%s_uniq", job->ref.al[a].name.c_str());
      fprintf(fu, "\n");
      size_t r = 0;
      for (auto &kv : table) {
        fprintf(fu, "%s", names[kv.first].c_str());
        for (size_t a = 0; a < A; ++a) fprintf(fu, "\t%lf", T.frac[r * A + a]);
        for (size_t a = 0; a < A; ++a) fprintf(fu, "\t%d", T.uniq[r * A + a]);
        fprintf(fu, "\n");
        ++r;
      }
      fclose(fu);
      if (barcodeEM) {
        std::vector<double> est;
        if (T.molecules.runEM(job, (uint32_t)table.size(), emPrior, est, true, "barcode EM on molecules") != T1K_OK) { fprintf(stderr, "analyzer: %s\n", t1k_job_last_error(job)); t1k_job_destroy(job); return EXIT_FAILURE; }
        if (!writeEstimates("_barcode_umi_em.tsv", est)) { t1k_job_destroy(job); return EXIT_FAILURE; }
      }
    }
  }
  logLine("Post analysis finishes.");
  t1k_job_destroy(job);
  return 0;
}


}  // extern "C"
