// Host-only driver of nn::gemm_plan() / nn::gemm_se_rows() (retto_amd/csrc/gemm_plan.cpp) for tests/test_gemm_plan_cpu.py.
// One query per stdin line, one answer per stdout line:
//   plan <variant> <dma> <split> <argmax_wide> <cus> <lda> <M> <K> <N> <Npad16> <ldc> <coff>
//        <am_max> <residual> <a_scale> <a_tab_stride> <act> <has_lab> <n_img> <ld_scale>
//     -> <kernel> <nt> <kg> <bf> <se> <grid_x> <grid_y> <label, or the error of an invalid plan>
//   se_rows <variant> <dma> <split> <lda> <M> <K> <N> <Npad16> <act> <min_pix>  ->  <rows>
// (am_max != 0 sets the CTC-head statistics with am_tiles = gemm_argmax_tiles(Npad16); a_scale != 0 sets a scale and a row table)
#include "nn.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace rt;

static const char* kernel_name(nn::GemmKernel k) {
  switch (k) {
    case nn::GemmKernel::none: return "none";
    case nn::GemmKernel::invalid: return "invalid";
    case nn::GemmKernel::split: return "split";
    case nn::GemmKernel::w: return "w";
    case nn::GemmKernel::dma: return "dma";
    case nn::GemmKernel::wide_256x240: return "wide_256x240";
    case nn::GemmKernel::wide_128x240: return "wide_128x240";
    case nn::GemmKernel::wide_128x128: return "wide_128x128";
    case nn::GemmKernel::stream: return "stream";
    case nn::GemmKernel::narrow: return "narrow";
    case nn::GemmKernel::argmax_256x240: return "argmax_256x240";
    case nn::GemmKernel::argmax_128x128: return "argmax_128x128";
    case nn::GemmKernel::argmax_narrow: return "argmax_narrow";
  }
  return "?";
}

int main() {
  static float dummy_f[4];
  static int dummy_i[4];
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    in >> op;
    if (op == "plan") {
      int cus, lda, K, N, Npad16, ldc, coff, am, res, asc;
      long long M;
      Epilogue e;
      in >> nn::g_gemm_variant >> nn::g_gemm_dma >> nn::g_gemm_split >> nn::g_argmax_wide >> cus >> lda >> M >> K >> N >> Npad16 >> ldc >>
          coff >> am >> res >> asc >> e.a_tab_stride >> e.act >> e.has_lab >> e.n_img >> e.ld_scale;
      if (!in) { printf("bad query\n"); return 2; }
      if (am) { e.am_max = dummy_f; e.am_idx = dummy_i; e.am_sum = dummy_f; e.am_tiles = nn::gemm_argmax_tiles(Npad16); }
      if (res) { e.residual = dummy_f; e.ld_res = ldc; }
      if (asc) { e.a_scale = dummy_f; e.a_tab = dummy_i; }
      const nn::GemmPlan p = nn::gemm_plan(lda, M, K, N, Npad16, ldc, coff, e, cus);
      printf("%s %d %d %d %d %u %u %s\n", kernel_name(p.kernel), p.nt, p.kg, (int)p.bf, (int)p.se, p.grid_x, p.grid_y,
             p.kernel == nn::GemmKernel::invalid ? p.error : p.label);
    } else if (op == "se_rows") {
      int lda, K, N, Npad16, act;
      long long M, min_pix;
      in >> nn::g_gemm_variant >> nn::g_gemm_dma >> nn::g_gemm_split >> lda >> M >> K >> N >> Npad16 >> act >> min_pix;
      if (!in) { printf("bad query\n"); return 2; }
      printf("%d\n", nn::gemm_se_rows(lda, M, K, N, Npad16, act, min_pix));
    } else if (!op.empty()) {
      printf("unknown query %s\n", op.c_str());
      return 2;
    }
    fflush(stdout);
  }
  return 0;
}
