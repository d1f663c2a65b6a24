// Which kernels run one LCNetV3 block (3x3 / 5x5 depthwise [-> squeeze-excite] -> 1x1 conv), decided on the host in one place
// (lc_plan.cpp): the fused thin-block kernel or none, the depthwise kernel with its strip layout, and whether the squeeze-excite
// is folded into the GEMM.  Plain C++ as gemm_plan.h: built and checked without a GPU (tests/test_lc_plan_cpu.py).
#pragma once
#include "common.h"

namespace rt {
namespace nn {

// Switches of the decision (read from the environment once, in lc_plan.cpp)
extern int g_lc_wave;    // RT_LC_WAVE: 3 = k_lc_lds for the thin blocks (default); 1 = the direct-load k_lc_wave on the stride-1 blocks
                         // (A/B); 0 = k_lc_thin / the unfused pair (rt_debug_set_variants bit 7)
extern int g_dw_sweep;   // RT_DW_SWEEP: column-sweep depthwise kernels on short maps (default 4; 0: off, rt_debug_set_variants bit 9)

constexpr int DW_SWEEP_POOL_STRIPS = 4;   // k_dwconv_sweep: strips of PR rows a pooled column may cross (LDS: 4 KB each)
constexpr int LC_THIN_TPB = 8;            // k_lc_thin: tiles per workgroup
constexpr int LC_WAVE_TPW = 4;            // k_lc_wave / k_lc_lds: tiles per wave (4 waves per workgroup)

// ---- depthwise conv ----
// k_dwconv_rows<K, R, SH, SW, pooled, lanes> as one number (dwconv()'s switch; the sweep instances are the numbers 1-6 below it)
constexpr int dw_rows_inst(int lanes, int K, int R, int sh, int sw) { return (((lanes * 8 + K) * 8 + R) * 4 + sh) * 4 + sw; }
enum class DwKernel {
  invalid,   // kernel size / stride without an instance: dwconv() throws
  rows32,    // k_dwconv_rows, 32-channel slabs (8 lanes per pixel)
  rows64,    // k_dwconv_rows, 64-channel slabs (16 lanes per pixel): wide tensors
  sweep,     // k_dwconv_sweep: short, wide maps, every input row fetched once
};
struct DwPlan {
  DwKernel kernel = DwKernel::invalid;
  int inst = 0;    // sweep: 1-6 (the table in lc_plan.cpp); rows32 / rows64: dw_rows_inst()
  // Strip layout: strips of R rows x 4 pixels, column-major per image, spb of them per partial sum of the fused squeeze-excite
  // pooling (`chunks` partials per image) -- the layout k_se_fc walks, whichever kernel writes it.
  int R = 0;       // output rows per strip
  int lanes = 0;   // lanes side by side on a pixel: 8 or 16
  int spb = 0;     // strips per workgroup of k_dwconv_rows = 256 / lanes
  int chunks = 0;
  unsigned grid_x = 0, grid_z = 0;   // (grid y = images)
};
// The kernel for a K x K depthwise conv, stride (sh, sw), channel pitch Cp, onto images of at most maxHo x maxWo pixels;
// pooled: it also leaves the squeeze-excite partial sums.
DwPlan dw_plan(int K, int sh, int sw, int Cp, int maxHo, int maxWo, bool pooled);

// ---- the block ----
// LC_UNFUSED: no fused form has an instance: nn::dwconv + nn::gemm.  (rt_debug_lc_block reports the values.)
enum LcRoute { LC_UNFUSED = 0, LC_THIN = 1, LC_WAVE = 2, LC_LDS = 3 };
struct LcShape {
  int K = 3, sh = 1, sw = 1;          // depthwise kernel size and stride
  int Cp = 0, C = 0;                  // input channel pitch, real channels
  int N = 0, Npad16 = 0;              // output channels of the pointwise conv, its packed width
  int dw_act = ACT_NONE, dw_has_lab = 0;   // depthwise tail
  bool se = false;                    // squeeze-excite between the two convs
  int maxHo = 0, maxWo = 0, ldy = 0;  // largest output image, output pitch
  long long rows = 0, min_pix = 0;    // output pixels of the level, of its smallest image
};
struct LcPlan {
  LcRoute route = LC_UNFUSED;
  // fused routes: the instance (LC_THIN: k_lc_thin 1-4, 6, 7; LC_WAVE: k_lc_wave 1-4; LC_LDS: k_lc_lds 1-4, 6-8 -- the tables in
  // lc_plan.cpp), the rows of its 16-pixel-wide tile (k_lc_thin TH, k_lc_lds / k_lc_wave MT) and the grid (y = images)
  int inst = 0, tile_h = 0;
  unsigned grid_x = 0;
  // LC_UNFUSED
  DwPlan dw;
  int se_rows = 0;   // row-block height of the squeeze-excite table folded into the GEMM (gemm_se_rows: 256 / 128); 0: not folded
};
// epi: the pointwise conv's epilogue (bias, activation, LAB; the caller makes the GEMM's own gemm_plan() once it is filled)
LcPlan lc_plan(const LcShape& s, const Epilogue& epi);

}  // namespace nn
}  // namespace rt
