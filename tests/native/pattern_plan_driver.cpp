// Host-only driver for the pattern part of rt::rec_tail_plan (retto_amd/csrc/rec_tail_plan.h), compiled with g++ by
// tests/test_pattern_cpu.py: no GPU.  One query per input line:
//   l0 l1 cand_k n_lines T.. n_pat (S P).. has_pat [pat..]
// pattern k has S states and P pairs (the plan reads nothing else of it).  One answer line each:
//   rows=.. z5=.. has_pat=.. max_P=.. max_S=.. bp_codes=.. plines=row0:T:pat:slot:bp,.. prows=..
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "rec_tail_plan.h"

using namespace rt;

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    int l0, l1, cand_k, n, n_pat, has;
    in >> l0 >> l1 >> cand_k >> n;
    std::vector<long long> off((size_t)n + 1, 0);
    for (int i = 0; i < n; i++) { long long T; in >> T; off[(size_t)i + 1] = off[(size_t)i] + T; }
    in >> n_pat;
    pt::Tables tb;
    for (int k = 0; k < n_pat; k++) { int S, P; in >> S >> P; tb.pats.push_back(pt::Pat{S, P, 0, 0, 0, 0, 0}); }
    in >> has;
    std::vector<int> pats((size_t)n, 0);
    for (int i = 0; has && i < n; i++) in >> pats[(size_t)i];
    if (!in) { printf("bad query\n"); continue; }
    const RecTailPlan p = rec_tail_plan(off.data(), l0, l1, nullptr, nullptr, lx::Tables(), nullptr, has ? pats.data() : nullptr, &tb);
    printf("rows=%lld z5=%d has_pat=%d max_P=%d max_S=%d bp_codes=%lld plines=", p.rows, (int)p.needs_z5(cand_k), (int)p.has_pat(), p.max_P,
           p.max_S, p.bp_codes);
    if (p.plines.empty()) printf("-");
    for (size_t i = 0; i < p.plines.size(); i++)
      printf("%s%d:%d:%d:%d:%lld", i ? "," : "", p.plines[i].row0, p.plines[i].T, p.plines[i].pat, p.plines[i].slot, p.plines[i].bp);
    printf(" prows=");
    if (p.prows.empty()) printf("-");
    for (size_t i = 0; i < p.prows.size(); i++) printf("%s%d", i ? "," : "", p.prows[i]);
    printf("\n");
  }
  return 0;
}
