// The kernels of one LCNetV3 block (lc_plan.h): the instance tables of the fused thin-block kernels and of the column-sweep
// depthwise kernel, the rules that pick among them, and the grids and strip layouts their launches use.
#include "lc_plan.h"

#include "gemm_plan.h"

namespace rt {
namespace nn {

int g_lc_wave = env_int("RT_LC_WAVE", 3);
int g_dw_sweep = env_int("RT_DW_SWEEP", 4);

namespace {

// k_dwconv_sweep<K, 16, 4, waves, SH, SW, pooled ? 3 : 0> instances (waves per SIMD of each: the kernel's header), by shape: the
// 5x5 stride-1 layers of the 12-row maps, the 3x3 stride-1 layer of the 128-channel maps (k_dwconv_rows fetched 1.33x its output
// there: 6-row patches of 4-row strips, PMC), and the recognition net's strided and squeeze-excite layers.  inst 0: none.
struct SweepInst { int K, sh, sw, min_ho, inst, inst_pooled; };
constexpr SweepInst SWEEPS[] = {{5, 1, 1, 5, 1, 3}, {3, 1, 1, 3, 2, 0}, {5, 2, 1, 3, 4, 5}, {3, 1, 2, 3, 6, 0}};

// k_lc_thin<C4, NT, TH, SH, SW>: (stride, C_in / 4, column tiles of 32) -> instance and tile rows.  Measured per shape: 64-pixel
// tiles (TH = 4: more workgroups per CU) win from 48 channels up, 128-pixel tiles below.
// ((2,1) 64 -> 128 of the rec net measured slower fused: 1.37 vs 1.05 ms)
struct ThinInst { int sh, sw, c4, nt32, inst, th; };
constexpr ThinInst THINS[] = {{1, 1, 4, 1, 1, 8},  {1, 1, 8, 2, 2, 8},                                    // 16 -> 32, 32 -> 64
                              {1, 1, 12, 2, 3, 4}, {1, 1, 16, 2, 4, 4},                                   // 48 -> 48, 64 -> 64
                              {2, 2, 8, 2, 6, 4},  {2, 2, 12, 3, 7, 4}};                                  // det s3.0: 32 -> 48, s4.0: 48 -> 96
// k_lc_wave / k_lc_lds: (stride, C_in, N) -> instance: the thin blocks of the two LCNetV3 backbones.  k_lc_wave has 1-4 only.
struct WaveInst { int sh, sw, Cp, Npad16, inst; };
constexpr WaveInst WAVES[] = {{1, 1, 16, 32, 1}, {1, 1, 32, 64, 2}, {1, 1, 48, 48, 3}, {1, 1, 64, 64, 4},
                              {2, 2, 32, 48, 6}, {2, 2, 48, 96, 7}, {2, 1, 64, 128, 8}};   // (8: rec s4.0)

int thin_inst(const LcShape& s, int* th) {
  if (s.K != 3 || s.Cp != round_up(s.C, 4)) return 0;
  for (const ThinInst& t : THINS)
    if (t.sh == s.sh && t.sw == s.sw && t.c4 * 4 == s.Cp && t.nt32 == (s.Npad16 + 31) / 32) { *th = t.th; return t.inst; }
  return 0;
}

int wave_inst(const LcShape& s, const Epilogue& epi) {
  if (s.K != 3 || s.Cp != s.C || s.N != s.Npad16) return 0;
  if (epi.residual || epi.a_scale || epi.am_max || !epi.bias || epi.act != ACT_HSWISH) return 0;
  // the pointwise half always ends in the LAB's fma: with a = 1, c = 0 it would turn the -0 hardswish gives below -3 into +0, one
  // bit away from k_lc_thin and the unfused pair (tests/test_gpu_rec_kernels.py); every block of the two backbones has the LAB
  if (!epi.has_lab) return 0;
  // depthwise tail (LearnableRepLayer: the activation is skipped when stride == 2; the rec net's (2, 1) is not 2)
  const bool plain_tail = s.sh == 2 && s.sw == 2;
  if (plain_tail ? (s.dw_act != ACT_NONE || s.dw_has_lab) : (s.dw_act != ACT_HSWISH || !s.dw_has_lab)) return 0;
  // k_lc_lds / k_lc_wave address an image through a 32-bit buffer offset, out-of-range marker 0x80000000: images up to 1 GB
  const long long in_bytes = (long long)(s.maxHo * s.sh + 2) * (s.maxWo * s.sw + 2) * s.Cp * 4;
  const long long out_bytes = (long long)s.maxHo * s.maxWo * s.ldy * 4;
  if (in_bytes >= (1ll << 30) || out_bytes >= (1ll << 30)) return 0;
  for (const WaveInst& w : WAVES)
    if (w.sh == s.sh && w.sw == s.sw && w.Cp == s.Cp && w.Npad16 == s.Npad16) return w.inst;
  return 0;
}

}  // namespace

DwPlan dw_plan(int K, int sh, int sw, int Cp, int maxHo, int maxWo, bool pooled) {
  DwPlan p;
  if ((K != 3 && K != 5) || sh < 1 || sh > 2 || sw < 1 || sw > 2) return p;
  // Output rows per thread of k_dwconv_rows: 4 (stride 1) or 2 (stride 2); 3 for the 3- and 6-row maps of the recognition net's
  // last stages, where 4-row (2-row) strips would leave a quarter of the lanes' rows empty (stride 2 onto 3 rows: 2-row strips
  // measured faster).  It is also the strip height of the squeeze-excite partial sums, whichever kernel writes them: the pooled
  // k_dwconv_sweep instances add the outputs strip by strip in k_dwconv_rows' order, so the value stays part of the results.
  p.R = (maxHo == 6 || (maxHo == 3 && sh == 1)) ? 3 : (sh == 1 ? 4 : 2);
  // 64-channel slabs (256 contiguous bytes per pixel and load) from 192 channels (5x5: 2.9 -> 4.1 TB/s on 256 channels) / 128
  // channels (3x3) up, for the shapes with a wide-slab instance; 32-channel slabs otherwise
  const bool wide = K == 5 ? Cp >= 192 && (sw == 1 || (sh == 2 && p.R == 2)) : Cp >= 128 && sh == 1 && p.R == 4 && !pooled;
  p.lanes = wide ? 16 : 8;
  p.spb = 256 / p.lanes;
  const int strips_x = (maxWo + 3) / 4, strips_y = (maxHo + p.R - 1) / p.R;
  p.chunks = (int)(((long long)strips_x * strips_y + p.spb - 1) / p.spb);
  p.grid_z = (unsigned)((Cp + p.lanes * 4 - 1) / (p.lanes * 4));
  // short, wide maps: one thread column sweeps the whole height.  Pooled: the partial sums keep the layout and the values of the row
  // kernel's 3-row strips, and a column's strips must fit the kernel's LDS.
  if (g_dw_sweep && wide && maxHo * sh <= 24)
    for (const SweepInst& s : SWEEPS)
      if (s.K == K && s.sh == sh && s.sw == sw && maxHo >= s.min_ho) {
        const bool pool3 = p.R == 3 && strips_y <= DW_SWEEP_POOL_STRIPS;
        p.inst = !pooled ? s.inst : pool3 ? s.inst_pooled : 0;
      }
  if (p.inst) {
    p.kernel = DwKernel::sweep;
    p.grid_x = (unsigned)((strips_x + p.spb - 1) / p.spb);
  } else {
    p.kernel = wide ? DwKernel::rows64 : DwKernel::rows32;
    p.inst = dw_rows_inst(p.lanes, K, p.R, sh, sw);
    p.grid_x = (unsigned)p.chunks;
  }
  return p;
}

LcPlan lc_plan(const LcShape& s, const Epilogue& epi) {
  LcPlan p;
  const int tiles_x = (s.maxWo + 15) / 16;
  auto fused = [&](LcRoute route, int inst, int tile_h, int tiles_per_block) {
    p.route = route; p.inst = inst; p.tile_h = tile_h;
    p.grid_x = (unsigned)((tiles_x * ((s.maxHo + tile_h - 1) / tile_h) + tiles_per_block - 1) / tiles_per_block);
    return p;
  };
  if (!s.se) {
    int th = 0;
    if (const int inst = g_lc_wave ? wave_inst(s, epi) : 0) {
      // LDS-staged form: 4-row tiles at stride 1 (2 waves per SIMD), 2-row tiles at stride 2.  The direct-load form (2-row tiles) is
      // kept for the stride-1 blocks only: A/B, RT_LC_WAVE=1.
      if (g_lc_wave >= 3 || inst >= 6) return fused(LC_LDS, inst, s.sh == 1 ? 4 : 2, 4 * LC_WAVE_TPW);
      return fused(LC_WAVE, inst, 2, 4 * LC_WAVE_TPW);
    }
    if (const int inst = thin_inst(s, &th)) return fused(LC_THIN, inst, th, LC_THIN_TPB);
  }
  // Squeeze-excite without extra passes over the depthwise output: the depthwise kernel leaves per-block channel sums, the FC turns
  // them into scales, and the pointwise GEMM multiplies them in while staging its A rows -- where the GEMM has such a form
  if (s.se && (s.K == 3 || s.K == 5))
    p.se_rows = gemm_se_rows(s.Cp, s.rows, round_up(s.C, 4), s.N, s.Npad16, epi.act, s.min_pix);
  p.dw = dw_plan(s.K, s.sh, s.sw, s.Cp, s.maxHo, s.maxWo, p.se_rows > 0);
  return p;
}

}  // namespace nn
}  // namespace rt
