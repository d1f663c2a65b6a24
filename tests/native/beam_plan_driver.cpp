// Host-only driver for the beam part of rt::rec_tail_plan (retto_amd/csrc/rec_tail_plan.h) and the host rule of ctc_beam.h,
// compiled with g++ -fsanitize=address,undefined by tests/test_beam_plan_cpu.py: no GPU.  One query per input line:
//   plan l0 l1 cand_k n_lines T.. beam nbest
//     -> rows=.. z5=.. has_beam=.. bnodes=.. fits=.. blines=row0:T:node0:slot:out,.. brows=..
//   beam N T beam nbest l[0][0] .. l[T-1][N-1]
//     the host rule over one line of integer logits (lse by lx::row_lse)
//     -> count=.. then per hypothesis " logprob:tok,tok,.." (":" alone: the empty string)
//   check beam nbest
//     -> ok   or   error: <bm::check_params' message>
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
    std::string op;
    in >> op;
    if (op == "plan") {
      int l0, l1, cand_k, n, beam, nbest;
      in >> l0 >> l1 >> cand_k >> n;
      std::vector<long long> off((size_t)n + 1, 0);
      for (int i = 0; i < n; i++) { long long T; in >> T; off[(size_t)i + 1] = off[(size_t)i] + T; }
      in >> beam >> nbest;
      if (!in) { printf("bad query\n"); continue; }
      const RecTailPlan p = rec_tail_plan(off.data(), l0, l1, nullptr, nullptr, lx::Tables(), nullptr, nullptr, nullptr, nullptr, nullptr,
                                          beam, nbest);
      printf("rows=%lld z5=%d has_beam=%d bnodes=%lld fits=%d blines=", p.rows, (int)p.needs_z5(cand_k), (int)p.has_beam(), p.bnodes,
             (int)p.bnodes_fit());
      if (p.blines.empty()) printf("-");
      for (size_t i = 0; i < p.blines.size(); i++)
        printf("%s%d:%d:%d:%d:%lld", i ? "," : "", p.blines[i].row0, p.blines[i].T, p.blines[i].lex, p.blines[i].slot, p.blines[i].out);
      printf(" brows=");
      if (p.brows.empty()) printf("-");
      for (size_t i = 0; i < p.brows.size(); i++) printf("%s%d", i ? "," : "", p.brows[i]);
      printf(" other=%d%d%d%d\n", (int)p.has_lex(), (int)p.has_pat(), (int)p.has_kw(), (int)!p.crows.empty());
    } else if (op == "beam") {
      int N, T, beam, nbest;
      in >> N >> T >> beam >> nbest;
      if (!in || N < 2 || T < 0 || bm::check_params(beam, nbest)) { printf("bad query\n"); continue; }
      // (exactly sized: the sanitizer sees every index the rule touches)
      std::vector<float> logits((size_t)T * N), lse((size_t)T);
      for (float& v : logits) in >> v;
      if (!in) { printf("bad query\n"); continue; }
      for (int t = 0; t < T; t++) lse[(size_t)t] = lx::row_lse(logits.data() + (size_t)t * N, N);
      std::vector<bm::Beam> out((size_t)nbest);
      std::vector<int32_t> tok((size_t)nbest * T, -1);
      const int count = bm::line_beams(logits.data(), N, lse.data(), T, N, beam, nbest, out.data(), tok.data());
      printf("count=%d", count);
      for (int k = 0; k < count; k++) {
        printf(" %.6f:", out[(size_t)k].logprob);
        for (int i = 0; i < out[(size_t)k].n_tokens; i++) printf("%s%d", i ? "," : "", tok[(size_t)k * T + i]);
      }
      printf("\n");
    } else if (op == "check") {
      int beam, nbest;
      in >> beam >> nbest;
      const char* why = bm::check_params(beam, nbest);
      printf("%s%s\n", why ? "error: " : "ok", why ? why : "");
    } else {
      printf("bad query\n");
    }
  }
  return 0;
}
