// oracle/ref_index_harness.cpp -- TEST INFRASTRUCTURE ONLY.  Tiny driver around the REFERENCE's own k-mer index (KmerIndex.hpp /
// KmerCode.hpp; compiled with -I$(REF) by oracle/Makefile `ref`, output oracle/_ref/index_harness; no reference source is
// copied): reads sequences, one per line (an empty line is an empty sequence), feeds each to KmerIndex::BuildIndexFromRead with its
// line number as id, and for every k-mer text of the second file (one per line, ACGT only) prints the list KmerIndex::Search returns
// as "allele:offset" pairs in list order, one line per k-mer (an empty line for an empty list).  tests/test_refindex_cpu.py pins
// tests/refindex_ref.py to it.
//   usage: index_harness SEQS.txt KMERS.txt K [N_CODE]     N_CODE: what nucToNum holds for 'N' (default -1 as in Genotyper.cpp; FastqExtractor.cpp has 0)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>
char nucToNum[26] = {0, -1, 1, -1, -1, -1, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 3, -1, -1, -1, -1, -1, -1};
char numToNuc[4] = {'A', 'C', 'G', 'T'};
#include "KmerIndex.hpp"

int main(int argc, char **argv) {
  if (argc < 4) { fprintf(stderr, "usage: index_harness SEQS.txt KMERS.txt K [N_CODE]\n"); return 1; }
  const int k = atoi(argv[3]);
  if (argc > 4) nucToNum['N' - 'A'] = (char)atoi(argv[4]);
  std::ifstream seqs(argv[1]), kmers(argv[2]);
  if (!seqs || !kmers) { fprintf(stderr, "index_harness: cannot open the inputs\n"); return 1; }
  KmerIndex index;
  KmerCode code(k);
  std::string line;
  int id = 0;
  while (std::getline(seqs, line)) {
    std::vector<char> s(line.begin(), line.end());
    s.push_back('\0');
    index.BuildIndexFromRead(code, s.data(), (int)line.size(), id++);
  }
  while (std::getline(kmers, line)) {
    if ((int)line.size() != k) { fprintf(stderr, "index_harness: '%s' is not a %d-mer\n", line.c_str(), k); return 1; }
    KmerCode q(k);
    for (char c : line) q.Append(c);
    SimpleVector<struct _indexInfo> &list = *index.Search(q);
    std::string out;
    for (int i = 0; i < list.Size(); ++i) out += (i ? " " : "") + std::to_string(list[i].idx) + ":" + std::to_string(list[i].offset);
    printf("%s\n", out.c_str());
  }
  return 0;
}
