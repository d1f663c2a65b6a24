// The fp32 GEMM kernel choice behind nn::gemm() (gemm_plan.h): the production rule, the size / alignment predicates of the
// persistent kernels, the forced variants of the kernel micro-benchmark, the template arguments and grids, and the profiler label.
#include "nn.h"

#include <algorithm>
#include <cstdlib>
#include <initializer_list>

namespace rt {
namespace nn {

int env_int(const char* name, int def) {
  const char* v = getenv(name);
  return v ? atoi(v) : def;
}

int g_gemm_variant = 0;
int g_gemm_dma = env_int("RT_GEMM_DMA", 1);   // A/B: 0 keeps the register-staged 256 x 240 tile
int g_gemm_split = env_int("RT_GEMM_SPLIT", 0);
int g_argmax_wide = 0;   // (measured: 128 x 128 wide tile 0.92 ms, 256 x 240 tile 0.97 ms)

int gemm_argmax_tiles(int Npad16) { return g_argmax_wide == 1 ? (Npad16 + 239) / 240 : (Npad16 + 127) / 128; }

namespace {

struct Env {   // read once, on the first plan
  int w = env_int("RT_GEMM_W", 1);          // A/B: 0 = k_gemm<8> instead of k_gemm32w
  int mid = env_int("RT_GEMM_MID", 1);      // A/B: 0 = the 128 x 240 tile from 16384 rows
  int occ = env_int("RT_GEMM_OCC", 2);      // narrow kernel: workgroups per CU to aim for
  int bf = env_int("RT_GEMM_BF", 1);        // A/B: 0 = k_gemm's pointer fetch
  int gs_only = env_int("RT_GS_ONLY", 3);   // (split triage: 1 = plain launches only, 2 = +se only)
};
const Env& env() {
  static const Env e;
  return e;
}

// production rule (tools/bench_gemm.py): 15 = 256 x 240 tile, 10 = 128 x 240 tile, 0 = narrow / streaming kernel
int production_variant(long long M, int Npad16) {
  if (Npad16 % 240 == 0 && M >= 131072) return 15;  // 256 x 240 tile: halves the weight re-fetch per row
  // (round 5: the 128 x 240 tile only where it fills the chip twice -- 38 k rows x 240 channels, a one-page batch, are 300
  //  workgroups of 768 threads on 256 CUs: two rounds for 1.17 rounds of work; the narrow kernel's 600 workgroups sit four to a CU)
  if (Npad16 % 240 == 0 && M >= 16384 && (!env().mid || (M + 127) / 128 * (Npad16 / 240) >= 512)) return 10;
  // (the 128 x 128 tile, variant 8, lost to the narrow kernel once that prefetched its next K-slab: 192 x 192 at
  // 115200 rows 85 vs 65 TFLOP/s, 128 x 128 at 2.4 M rows 76 vs 72; it remains the squeeze-excite (a_scale) and CTC tile)
  return 0;
}

// k_gemm32w: K = N = 128 with the weights resident in LDS
bool w_fits(int lda, long long M, int K, int N, int Npad16, const Epilogue& epi, int ldc, int coff) {
  if (!env().w || epi.am_max || epi.residual || epi.a_scale) return false;
  if (K != 128 || N != 128 || Npad16 != 128) return false;
  if (lda < 128 || (lda & 3) || (long long)lda * 4 * W_BM >= (1ll << 31)) return false;
  if ((ldc & 3) || (coff & 3)) return false;   // 16-byte stores of four consecutive channels
  return M >= 65536;
}

// k_gemm32p: N a multiple of 240, K whole 16-deep groups, plain bias / activation / LAB epilogue or the 3-int squeeze-excite table
bool dma_fits(int lda, long long M, int K, int N, int Npad16, const Epilogue& epi) {
  if (epi.am_max || epi.residual) return false;
  // squeeze-excite scale: 3-int row-block table, hardswish epilogue, K within the LDS scale table
  if (epi.a_scale && (epi.a_tab_stride != 3 || !epi.a_tab || K > P_SCK || epi.act != ACT_HSWISH || epi.n_img <= 0)) return false;
  if ((N + 3) / 4 * 4 != N) return false;
  if (Npad16 != N || N % P_BN != 0 || N > P_BIAS_MAX) return false;
  // (>= 4 slabs: the request side reads the next tile's id when it has issued a tile's last slab, at the hand-over of the
  //  tile's slab nkc - 3; the id is published at the hand-over of slab 1)
  if (K % 16 != 0 || K <= 3 * KC || lda < round_up(K, KC) || (lda & 3)) return false;   // whole 16-deep groups; 32-deep slabs readable
  if ((long long)lda * 4 * P_BM >= (1ll << 31)) return false;
  return M >= P_BM;
}

// k_gemm_split: the same layers, either squeeze-excite table
bool split_fits(int lda, long long M, int K, int N, int Npad16, const Epilogue& epi, int ldc, int coff) {
  if (epi.am_max || epi.residual) return false;
  if (!(env().gs_only & (epi.a_scale ? 2 : 1))) return false;
  // squeeze-excite scale: a row-block table of either form, hardswish epilogue, images of >= 128 rows (what gemm_se_rows() > 0 says)
  if (epi.a_scale && (!epi.a_tab || (epi.a_tab_stride != 2 && epi.a_tab_stride != 3) || epi.act != ACT_HSWISH || epi.n_img <= 0 || epi.ld_scale < K)) return false;
  if (Npad16 != N || N % S_BN != 0 || N > 960) return false;
  if (lda < round_up(K, KC) || (lda & 3)) return false;          // whole 32-deep slabs readable (padding channels hold zeros)
  if ((long long)lda * 4 * 32 >= (1ll << 31)) return false;
  if ((ldc & 3) || (coff & 3)) return false;   // 16-byte stores of four consecutive channels
  // (large launches only: the small-batch dispatch of a one-page call stays on the narrow fp32 kernel)
  return M >= 32768 && K > 3 * KC;   // (>= 4 slabs: the request streams read the next tile's id two slabs before a tile ends; it is published in the tile's first slab)
}

// buffer-resource fetch of k_gemm (k_gemm<NT, *, true>): a tile's 128 rows and the packed weights within the 2-GB offset range
bool bf_fits(int lda, int K, int Npad16) {
  return env().bf && (long long)128 * lda * 4 < (1ll << 31) && (long long)((K + KC - 1) / KC) * Npad16 * KC * 4 < (1ll << 31);
}

// the first of `sizes` that holds n, else the last
int bucket(int n, std::initializer_list<int> sizes) {
  for (int s : sizes)
    if (n <= s) return s;
  return *(sizes.end() - 1);
}

GemmPlan plan(int lda, long long M, int K, int N, int Npad16, int ldc, int coff, const Epilogue& epi, int cus, bool split_on) {
  GemmPlan p;
  auto take = [&](GemmKernel k, const char* label, long long gx = 0, long long gy = 0) {
    p.kernel = k; p.label = label; p.grid_x = (unsigned)gx; p.grid_y = (unsigned)gy;
    return p;
  };
  auto fail = [&](const char* why) {
    p.kernel = GemmKernel::invalid; p.error = why; p.se = false;
    return p;
  };
  const long long rb128 = (M + 127) / 128, rb256 = (M + 255) / 256;
  const int cb128 = (Npad16 + 127) / 128, cb240 = (Npad16 + 239) / 240;
  if (M <= 0) return take(GemmKernel::none, "gemm_pw/none");
  if (epi.am_max) {  // CTC head: softmax statistics per column tile instead of the logits (argmax_merge folds them)
    if (epi.am_tiles != gemm_argmax_tiles(Npad16)) return fail("gemm: am_tiles must be gemm_argmax_tiles(Npad16)");
    if (g_argmax_wide == 1) return take(GemmKernel::argmax_256x240, "gemm_ctc_fc", rb256, cb240);
    if (g_argmax_wide == 2) return take(GemmKernel::argmax_128x128, "gemm_ctc_fc", rb128, cb128);
    p.nt = 8; p.bf = bf_fits(lda, K, Npad16);   // narrow kernel, 128-column blocks
    return take(GemmKernel::argmax_narrow, "gemm_ctc_fc", rb128, cb128);
  }
  const int forced = g_gemm_variant;
  int v = forced ? forced : production_variant(M, Npad16);
  if ((v == 40 || (!forced && split_on)) && split_fits(lda, M, K, N, Npad16, epi, ldc, coff)) {
    p.se = epi.a_scale != nullptr;
    return take(GemmKernel::split, p.se ? "gemm_pw/k_gemm_split+se" : "gemm_pw/k_gemm_split");
  }
  if (v == 40) v = 30;
  if (!forced && w_fits(lda, M, K, N, Npad16, epi, ldc, coff)) return take(GemmKernel::w, "gemm_pw/k_gemm32w");
  // persistent LDS-DMA form of the 256 x 240 tile (variant 30; production for the large N = 240 / 480 layers)
  if ((v == 30 || (v == 15 && !forced && g_gemm_dma)) && dma_fits(lda, M, K, N, Npad16, epi)) {
    p.se = epi.a_scale != nullptr;
    return take(GemmKernel::dma, p.se ? "gemm_pw/k_gemm32p+se" : "gemm_pw/k_gemm32p");
  }
  if (v == 30) v = 15;
  if (epi.a_scale) {  // squeeze-excite scale folded into the A staging of the register-staged wide tiles
    if (epi.a_tab_stride != 2) return fail("gemm: a 3-int a_tab is only understood by k_gemm32p (gemm_se_rows() == 256)");
    if (K > 512 || !epi.a_tab) return fail("gemm: a_scale needs K <= 512 and a row-tile table");
    if (v == 15) v = 10;  // the 256-row tile has no registers to spare for the scaling (spills): 128 x 240 measured faster
    if (v == 0 && Npad16 >= 128 && M >= 8192) v = 8;   // (the 128 x 128 tile in place of the narrow kernel)
    if (v != 10 && v != 8) return fail("gemm: a_scale is only implemented for the wide tiles");
    p.se = true;
    if (v == 10) return take(GemmKernel::wide_128x240, "gemm_pw/k_gemm_wide<2,5,4,3>+se", rb128, cb240);
    return take(GemmKernel::wide_128x128, "gemm_pw/k_gemm_wide<2,4,4,2>+se", rb128, cb128);
  }
  if (v == 8) return take(GemmKernel::wide_128x128, "gemm_pw/k_gemm_wide<2,4,4,2>", rb128, cb128);
  if ((v == 20 && Npad16 <= 128 && K <= 128) || (v == 0 && Npad16 <= 64 && K <= 64 && M >= 65536)) {  // streaming kernel for the thin layers
    p.nt = bucket(Npad16 / 16, {1, 2, 3, 4, 6, 8});
    p.kg = bucket((K + 15) / 16, {1, 2, 4, 6, 8});
    const long long tiles = (M + 31) / 32;
    return take(GemmKernel::stream, "gemm_pw/thin", std::min<long long>((tiles + 3) / 4, 256 * 8), 1);
  }
  if (v == 15) return take(GemmKernel::wide_256x240, "gemm_pw/k_gemm_wide<4,5,4,3>", rb256, cb240);
  if (v == 10) return take(GemmKernel::wide_128x240, "gemm_pw/k_gemm_wide<2,5,4,3>", rb128, cb240);
  // narrow kernel: 16 * NT columns per workgroup
  const int ntiles = Npad16 / 16;
  int nt = ntiles >= 8 ? 8 : ntiles;
  if (ntiles > 8) {  // pick the split with least padding among 8 / 6 / 5 / 4
    int waste = round_up(ntiles, 8) - ntiles;
    for (int c : {6, 5, 4}) {
      const int w = round_up(ntiles, c) - ntiles;
      if (w < waste) { waste = w; nt = c; }
    }
  }
  // small M (one page, the coarse pyramid levels): fewer columns per workgroup until there is a workgroup per CU -- 3600 x 480 x
  // 480 on 128 x 128 tiles is 116 workgroups walking 15 slabs each, 35 us; the column tiles are independent: same bits
  const long long want = (long long)cus * env().occ;
  while (nt > 1 && rb128 * ((ntiles + nt - 1) / nt) < want) nt = (nt + 1) / 2;
  p.nt = nt; p.bf = bf_fits(lda, K, Npad16);
  return take(GemmKernel::narrow, "gemm_pw/thin", rb128, (ntiles + nt - 1) / nt);
}

}  // namespace

GemmPlan gemm_plan(int lda, long long M, int K, int N, int Npad16, int ldc, int coff, const Epilogue& epi, int cus) {
  return plan(lda, M, K, N, Npad16, ldc, coff, epi, cus, g_gemm_split != 0);
}

int gemm_se_rows(int lda, long long M, int K, int N, int Npad16, int act, long long min_pix) {
  // forced variants take no fused form; every image must cover a 128-row block (a 256-row block then spans at most three images)
  if (g_gemm_variant || min_pix < 128) return 0;
  static const float scale = 0.f;
  static const int tab = 0;
  Epilogue probe;
  probe.act = act; probe.a_scale = &scale; probe.ld_scale = lda; probe.a_tab = &tab; probe.n_img = 1;
  for (const int stride : {3, 2}) {
    probe.a_tab_stride = stride;
    if (plan(lda, M, K, N, Npad16, chan_pitch(N), 0, probe, 0, false).se) return stride == 3 ? 256 : 128;
  }
  return 0;
}

}  // namespace nn
}  // namespace rt
