// Which fp32 GEMM kernel nn::gemm() launches, decided on the host in one place (gemm_plan.cpp).  Plain C++: no HIP API
// calls, so that the decision can be built and checked without a GPU (tests/test_gemm_plan_cpu.py).
#pragma once
#include "common.h"

namespace rt {
namespace nn {

// Switches of the decision (defaults in gemm_plan.cpp; the RT_GEMM_W / _MID / _OCC / _BF and RT_GS_ONLY environment variables are
// read there once).
extern int g_gemm_variant;  // kernel micro-benchmark hook (rt_bench_gemm): 0 = production choice; 1 narrow, 8 / 10 / 15 wide tiles,
                            // 20 streaming, 30 k_gemm32p, 40 k_gemm_split (falling back 40 -> 30 -> 15 where a form does not apply)
extern int g_gemm_dma;      // A/B: persistent LDS-DMA wide GEMM on (default) / off
extern int g_gemm_split;    // opt-in: split-bf16 form of the wide layers (RT_GEMM_SPLIT=1, rt_debug_set_variants flag bit 12)
extern int g_argmax_wide;   // CTC head: 0 = narrow kernel with 128-column blocks; 2 = 128 x 128 wide tile; 1 = 256 x 240 tile

int env_int(const char* name, int def);   // an integer switch of the environment, or its default

// tile sizes the size predicates of the persistent kernels depend on
constexpr int P_BM = 256, P_BN = 240;   // k_gemm32p (nn_gemm_dma.hip)
constexpr int P_BIAS_MAX = 960;         // k_gemm32p: bias vector kept in LDS (N <= 960)
constexpr int P_SCK = 512;              // k_gemm32p + se: K <= 512 (scale table in LDS)
constexpr int W_BM = 64;                // k_gemm32w (nn_gemm_dma.hip)
constexpr int S_BN = 240;               // k_gemm_split (nn_gemm_split.hip)

enum class GemmKernel {
  none,            // M <= 0: nothing to launch
  invalid,         // no kernel takes the call: GemmPlan::error says why
  split,           // k_gemm_split (+se): gemm_split()
  w,               // k_gemm32w: gemm_w()
  dma,             // k_gemm32p (+se): gemm_dma()
  wide_256x240,    // k_gemm_wide<4,5,4,3>
  wide_128x240,    // k_gemm_wide<2,5,4,3> (+se)
  wide_128x128,    // k_gemm_wide<2,4,4,2> (+se)
  stream,          // k_gemm_stream<nt, kg>
  narrow,          // k_gemm<nt> (bf: buffer-resource fetch)
  argmax_256x240,  // CTC head (Epilogue::am_*): k_gemm_wide<4,5,4,3,0,0,0,1>
  argmax_128x128,  //   k_gemm_wide<2,4,4,2,0,0,0,1>
  argmax_narrow,   //   k_gemm<8,1> (bf)
};

struct GemmPlan {
  GemmKernel kernel = GemmKernel::invalid;
  bool se = false;               // the squeeze-excite scale (Epilogue::a_scale) is folded into the A staging
  int nt = 0, kg = 0;            // k_gemm<nt>; k_gemm_stream<nt, kg>
  bool bf = false;               // k_gemm<nt, *, true>
  unsigned grid_x = 0, grid_y = 0;   // register-staged wide tiles, stream and narrow kernels (the persistent ones size their own)
  const char* label = nullptr;   // profiler label of a pointwise-conv GEMM that runs this kernel
  const char* error = nullptr;   // kernel == invalid
};

// The kernel for C[M, ldc] (+coff) = epi(A[M, lda] x W) with W packed for Npad16 columns; cus = CUs of the launch stream.
GemmPlan gemm_plan(int lda, long long M, int K, int N, int Npad16, int ldc, int coff, const Epilogue& epi, int cus);
// Row-block height of the squeeze-excite (a_scale) table the fp32 kernels accept for this layer, asked before the table is built:
// 256 (k_gemm32p: 3 ints per 256-row block, Epilogue::a_tab_stride = 3, n_img set), 128 (register-staged wide tiles: 2 ints per
// 128-row block) or 0 (no fused form: scale the tensor in a pass of its own).  min_pix: rows of the smallest image.  The split
// kernel accepts either table, so the answer does not depend on g_gemm_split.
int gemm_se_rows(int lda, long long M, int K, int N, int Npad16, int act, long long min_pix);

}  // namespace nn
}  // namespace rt
