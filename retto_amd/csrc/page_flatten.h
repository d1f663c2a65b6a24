// Page flatten: every channel of a page divided by the paper level estimated around each pixel (flat-fielding, the "scanner app"
// filter), before anything else reads the page.  Written once for the gfx950 kernels (page_flatten.hip), the CPU restatement
// (flatten_page_host below: rt_debug_flatten_page_host) and the session (flatten_pages: session.cpp).  A photographed page with a
// shadow across it or under a coloured lamp is not served by equalisation (page_enhance.h): a shadow edge inside a tile stays an
// edge, the texture of the dark half is amplified, and a colour cast stays because only the luma moves.  Dividing by the level
// makes paper white, keeps the relative darkness of ink, and removes the illumination gradient and the cast.  It is the partner
// of page enhance: with both on a page is flattened first and what is left is equalised, enhance(flatten(page)).  The reference has
// no counterpart; the rule here is this project's own.  All arithmetic is 32-bit integer, so the kernels, the CPU restatement and
// a test's reference agree byte for byte.
//
// Setting.  rt_set_page_flatten(s, radius, floor), per session.  radius = 0: off, the initial state (floor is then not looked
// at).  Otherwise 1 <= radius <= 16 (in cells) and 1 <= floor <= 255.  Anything else: RT_ERR_INVALID naming the parameter.
//
// The rule, for a page of h x w RGB8 pixels, r = radius, f = floor; each of the three channels on its own:
//   1. Cells.  gh = ceil(h / 4), gw = ceil(w / 4); P[gy][gx] = the maximum of the channel over the pixels 4 gy <= y < min(h, 4 gy + 4),
//      4 gx <= x < min(w, 4 gx + 4).  Edge cells are partial, nothing is padded.
//   2. Closing.  D[gy][gx] = max of P[j][i] over |j - gy| <= r, |i - gx| <= r clipped to the grid; C[gy][gx] = min of D over the
//      same clipped window.  A stroke narrower than the window leaves no trace; the paper around it does.
//   3. Smoothing.  S = sum of C over the same clipped window, n = its number of cells, B = (S + n / 2) / n (box_mean).
//   4. Level at a pixel: the bilinear blend of B at the cell centres.  Along an axis of g cells, coordinate i gives u = 2 i - 3;
//      g == 1 or u <= 0: (i0, i1, wt) = (0, 0, 0); otherwise i0 = u / 8, and i0 >= g - 1: (g - 1, g - 1, 0), else
//      (i0, i0 + 1, u - 8 i0) (axis).  L = (8 - wy) ((8 - wx) B[y0][x0] + wx B[y0][x1]) + wy ((8 - wx) B[y1][x0] + wx B[y1][x1]),
//      the level in 1 / 64 units (level).
//   5. Divide.  L = max(L, 64 f); out = min(255, (p * 16320 + L / 2) / L), 16320 = 255 * 64 (flat_value).  The floor keeps large
//      dark areas (photographs, black bars) from being blown up to noise; a channel equal to its own level maps to 255.
// The output is always a new buffer; a caller's RT_MEM_DEVICE page is never written.
//
// Not supported: per-page or per-region settings; flattening in rt_resize_both, rt_det_preprocess or rt_crop_images, which take
// the page as it is.
// What is not claimed: that flattened pages are read better.  The weights here are synthetic; the effect on recognition accuracy
// with trained PP-OCRv4 weights has not been measured.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>
#include "geom_math.h"

namespace rt {
class Profiler;   // runtime.h
namespace pf {

constexpr int CELL = 4, MAX_RADIUS = 16, LEVEL_ONE = 64, NUM = 255 * LEVEL_ONE;

// nullptr when (radius, floor) is accepted, else what is wrong with it; radius = 0 is "off" whatever floor is
inline const char* check_params(int radius, int floor) {
  if (radius == 0) return nullptr;
  if (radius < 1 || radius > MAX_RADIUS) return "radius must be 0 (off) or in [1, 16]";
  if (floor < 1 || floor > 255) return "floor must be in [1, 255]";
  return nullptr;
}

RT_HD int cells_along(int n) { return (n + CELL - 1) / CELL; }
RT_HD int box_mean(int sum, int n) { return (sum + n / 2) / n; }
// the two cells and the weight of the second along one direction, for pixel coordinate i of g cells
struct Axis { int i0, i1, w; };
RT_HD Axis axis(int i, int g) {
  const int u = 2 * i - 3;
  if (g == 1 || u <= 0) return Axis{0, 0, 0};
  const int i0 = u / 8;
  if (i0 >= g - 1) return Axis{g - 1, g - 1, 0};
  return Axis{i0, i0 + 1, u - 8 * i0};
}
RT_HD int level(int wx, int wy, int b00, int b01, int b10, int b11) {
  return (8 - wy) * ((8 - wx) * b00 + wx * b01) + wy * ((8 - wx) * b10 + wx * b11);
}
RT_HD int floored(int L, int floor) { return L > LEVEL_ONE * floor ? L : LEVEL_ONE * floor; }
RT_HD int flat_value(int p, int L) { const int q = (p * NUM + L / 2) / L; return q < 255 ? q : 255; }
// flat_value with a float reciprocal of L in place of the division, as k_flatten_apply computes it: rcp = 1 / L to within one
// unit in the last place (v_rcp_f32).  N = p * 16320 + L / 2 < 2^23 and L are exact in fp32; the product's relative error is below
// 2^-22 and N / L < 65026, so the truncated quotient is off by at most one either way, which the remainder corrects exactly.
RT_HD int flat_value_rcp(int p, int L, float rcp) {
  const int N = p * NUM + L / 2;
  int q = (int)((float)N * rcp);
  const int rem = N - q * L;
  q += (rem >= L ? 1 : 0) - (rem < 0 ? 1 : 0);
  return q < 255 ? q : 255;
}

// ---- the kernels' descriptors (page_flatten.hip): one per page of a lane part ----------------------------------------------
// src: the page (h x w RGB8, rows of 3 w bytes), dst: the flattened page, cells / base: the planes P / B, [3][gh] rows of gp bytes
// each, gp = gw rounded up to a dword so that k_flatten_level stages rows of P with dword loads (16-byte aligned planes).
// strip_base / tile_base / block_base: the page's first entry in the part's flat lists of pool strips (a row of cells cut into
// POOL_CELLS-cell pieces), level tiles (TILE x TILE cells, times three channels) and apply blocks (APPLY_H x APPLY_W pixels).  Every
// page has at least one of each, so the bases strictly increase: entry g belongs to the last page whose base is <= g.
constexpr int POOL_CELLS = 256, TILE = 32, APPLY_W = 128, APPLY_H = 32;
struct DevPage {
  const uint8_t* src; uint8_t* dst; uint8_t* cells; uint8_t* base;
  int h, w, gh, gw, gp, strips_x, tiles_y, tiles_x, blocks_y, blocks_x;
  uint32_t strip_base, tile_base, block_base;
};
// fills the geometry and the bases of pages[0 .. n) from their h / w; returns false when a list would pass 2^31 - 1 entries
inline bool plan_pages(DevPage* pages, int n) {
  uint64_t strips = 0, tiles = 0, blocks = 0;
  for (int i = 0; i < n; i++) {
    DevPage& p = pages[i];
    p.gh = cells_along(p.h); p.gw = cells_along(p.w); p.gp = (p.gw + 3) & ~3;
    p.strips_x = (p.gw + POOL_CELLS - 1) / POOL_CELLS;
    p.tiles_y = (p.gh + TILE - 1) / TILE; p.tiles_x = (p.gw + TILE - 1) / TILE;
    p.blocks_y = (p.h + APPLY_H - 1) / APPLY_H; p.blocks_x = (p.w + APPLY_W - 1) / APPLY_W;
    p.strip_base = (uint32_t)strips; p.tile_base = (uint32_t)tiles; p.block_base = (uint32_t)blocks;
    strips += (uint64_t)p.gh * p.strips_x; tiles += 3ull * p.tiles_y * p.tiles_x; blocks += (uint64_t)p.blocks_y * p.blocks_x;
    if (strips > 0x7fffffffu || tiles > 0x7fffffffu || blocks > 0x7fffffffu) return false;
  }
  return true;
}
#ifdef __HIPCC__
// the three launches over pages[0 .. n) (d_pages: their copy on the device), on st: k_flatten_pool over the flat list of strips,
// k_flatten_level over the tiles, k_flatten_apply over the blocks; prof (or null): the families page_flatten_pool / _level / _apply
void launch(hipStream_t st, Profiler* prof, const DevPage* d_pages, const DevPage* pages, int n, int radius, int floor);
#endif

// ---- the rule on the CPU, in plain loops ------------------------------------------------------------------------------------
// out [h * w * 3]; level_out (or null) [3 * gh * gw]: B
inline void flatten_page_host(const uint8_t* rgb, int h, int w, int radius, int floor, uint8_t* out, uint8_t* level_out) {
  const int gh = cells_along(h), gw = cells_along(w), r = radius;
  const size_t plane = (size_t)gh * gw;
  std::vector<uint8_t> own(level_out ? 0 : 3 * plane);
  uint8_t* B = level_out ? level_out : own.data();
  std::vector<int> P(plane), D(plane), Cl(plane);
  for (int ch = 0; ch < 3; ch++) {
    for (int gy = 0; gy < gh; gy++)
      for (int gx = 0; gx < gw; gx++) {
        int m = 0;
        for (int y = CELL * gy; y < h && y < CELL * gy + CELL; y++)
          for (int x = CELL * gx; x < w && x < CELL * gx + CELL; x++) { const int v = rgb[((size_t)y * w + x) * 3 + ch]; if (v > m) m = v; }
        P[(size_t)gy * gw + gx] = m;
      }
    for (int pass = 0; pass < 3; pass++)   // D = max of P, Cl = min of D, B = mean of Cl, each over the window clipped to the grid
      for (int gy = 0; gy < gh; gy++)
        for (int gx = 0; gx < gw; gx++) {
          const int j0 = gy - r > 0 ? gy - r : 0, j1 = gy + r < gh - 1 ? gy + r : gh - 1;
          const int i0 = gx - r > 0 ? gx - r : 0, i1 = gx + r < gw - 1 ? gx + r : gw - 1;
          int acc = pass == 1 ? 255 : 0;
          for (int j = j0; j <= j1; j++)
            for (int i = i0; i <= i1; i++) {
              const size_t at = (size_t)j * gw + i;
              if (pass == 0) { if (P[at] > acc) acc = P[at]; }
              else if (pass == 1) { if (D[at] < acc) acc = D[at]; }
              else acc += Cl[at];
            }
          const size_t at = (size_t)gy * gw + gx;
          if (pass == 0) D[at] = acc; else if (pass == 1) Cl[at] = acc;
          else B[ch * plane + at] = (uint8_t)box_mean(acc, (j1 - j0 + 1) * (i1 - i0 + 1));
        }
  }
  for (int y = 0; y < h; y++) {
    const Axis ay = axis(y, gh);
    for (int x = 0; x < w; x++) {
      const Axis ax = axis(x, gw);
      for (int ch = 0; ch < 3; ch++) {
        const uint8_t* b = B + ch * plane;
        const int L = level(ax.w, ay.w, b[(size_t)ay.i0 * gw + ax.i0], b[(size_t)ay.i0 * gw + ax.i1], b[(size_t)ay.i1 * gw + ax.i0],
                            b[(size_t)ay.i1 * gw + ax.i1]);
        const size_t at = ((size_t)y * w + x) * 3 + ch;
        out[at] = (uint8_t)flat_value(rgb[at], floored(L, floor));
      }
    }
  }
}

}  // namespace pf
}  // namespace rt
