// oracle/ref_seed_harness.cpp -- TEST INFRASTRUCTURE ONLY.  Tiny driver around the REFERENCE's own seeding (SeqSet.hpp; compiled with
// -I/root/reference by oracle/Makefile `ref`, output oracle/_ref/seed_harness; no reference source is copied): loads a FASTA with
// SeqSet::InputRefFa and, for every read on stdin (one per line), calls GetHitsFromRead(read, rc, 0, -1, false, hits, NULL) the way
// GetOverlapsFromRead does and prints one line: the hit count, then the distinct "strand:offset" pairs in the order the hits were made
// (strand 0 = the read as given, 1 = its reverse complement).  tests/test_seed_cpu.py pins tests/seed_ref.py to it.
//   usage: seed_harness REF.fa K [N_CODE]     N_CODE: what nucToNum holds for 'N' (default -1 as in Genotyper.cpp; FastqExtractor.cpp has 0)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
char nucToNum[26] = {0, -1, 1, -1, -1, -1, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 3, -1, -1, -1, -1, -1, -1};
char numToNuc[4] = {'A', 'C', 'G', 'T'};
#include "SeqSet.hpp"

int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "usage: seed_harness REF.fa K [N_CODE]\n"); return 1; }
  const int k = atoi(argv[2]);
  if (argc > 3) nucToNum['N' - 'A'] = (char)atoi(argv[3]);
  SeqSet set(k);
  set.InputRefFa(argv[1]);
  static char read[1 << 16];
  std::vector<char> rc(1 << 16);
  while (scanf("%65535s", read) == 1) {
    const int len = (int)strlen(read);
    if (len < k) { printf("0\n"); continue; }  // GetOverlapsFromRead returns before seeding (SeqSet.hpp:1598-1599)
    SimpleVector<struct _hit> hits;
    const int n = set.GetHitsFromRead(read, rc.data(), 0, -1, false, hits, NULL);
    std::string line = std::to_string(n);
    int ps = 0, po = -1;
    for (int i = 0; i < n; ++i) {
      const int s = hits[i].strand == 1 ? 0 : 1, o = hits[i].readOffset;
      if (i == 0 || s != ps || o != po) line += " " + std::to_string(s) + ":" + std::to_string(o);
      ps = s; po = o;
    }
    printf("%s\n", line.c_str());
  }
  return 0;
}
