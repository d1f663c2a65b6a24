// Page enhance: tile-wise contrast-limited histogram equalisation (CLAHE) of a page's luma before anything else reads the page.
// Written once for the gfx950 kernels (page_enhance.hip), the CPU restatement (enhance_page_host below: rt_debug_enhance_page_host)
// and the session (enhance_pages: session.cpp).  A faded receipt, a pencil form, a page with a shadow across it reach resize_both,
// the detector and the crops exactly as they arrived; the usual remedy in document OCR is CLAHE of the luma, which callers do on
// the host today -- one more pass over pages that are otherwise only uploaded, and impossible for RT_MEM_DEVICE pages and for
// pages decoded on the device.  The reference has no counterpart; the rule here is this project's own.  All arithmetic is 32-bit
// integer, so the kernels, the CPU restatement and a test's reference agree bit for bit.
//
// Setting.  rt_set_page_enhance(s, tile, clip), per session.  tile = 0: off, the initial state (clip is then not looked at).
// Otherwise tile is a multiple of 32 with 32 <= tile <= 512 and clip is finite with 1 <= clip <= 64; clip is held as
// clip_x16 = lrintf(clip * 16).  Anything else: RT_ERR_INVALID naming the parameter.
//
// The rule, for a page of h x w RGB8 pixels and t = tile:
//   1. Luma.  Y = (77 R + 150 G + 29 B + 128) >> 8.
//   2. Tiles.  nty = ceil(h / t), ntx = ceil(w / t); tile (ty, tx) covers rows [ty t, min(h, ty t + t)), the columns likewise.
//      Edge tiles are partial: `area` is a tile's real pixel count, nothing is padded or reflected.
//   3. Histogram and clipping, per tile.  hist[256] over Y; L = max(1, (clip_x16 * area) >> 12); excess = sum(max(0, hist[i] - L)),
//      hist[i] = min(hist[i], L); every bin gains excess / 256, and with r = excess % 256 the bins (k * 256) / r, k = 0 .. r - 1,
//      gain one more each (bin_gain).  The bins sum to `area` again.
//   4. LUT, per tile.  c[i] = the inclusive prefix sum; LUT[i] = (c[i] * 255 + area / 2) / area, a byte.
//   5. Interpolation, per pixel (x, y).  Tile centres are at (tx + 0.5) t.  Along x, u = 2 x + 1 - t; ntx == 1 or u <= 0:
//      tx0 = tx1 = 0, wx = 0; otherwise tx0 = u / (2 t), and tx0 >= ntx - 1: tx0 = tx1 = ntx - 1, wx = 0, else tx1 = tx0 + 1,
//      wx = u - 2 t tx0 (axis).  y likewise.  With a_rc = LUT[ty_r][tx_c][Y],
//        Y' = ((2t - wy) ((2t - wx) a00 + wx a01) + wy ((2t - wx) a10 + wx a11) + 2 t t) / (4 t t)
//      whose numerator is at most 4 * 512 * 512 * 255 + 2 * 512 * 512 < 2^31 (blend).
//   6. Colour.  d = Y' - Y; each of R, G, B becomes clamp(v + d, 0, 255): a grey page stays grey, chroma differences are kept.
// The output is always a new buffer; a caller's RT_MEM_DEVICE page is never written.
//
// Cells.  Between four neighbouring tile centres lies a t x t square, the tile grid shifted by t / 2: cell (cy, cx) covers the
// rows [cy t - t / 2, cy t + t / 2) and the columns likewise, clipped to the page.  For every pixel of a cell, axis() gives the same
// tiles -- cx = 0: tile 0 alone, 1 <= cx <= ntx - 1: tiles cx - 1 and cx, cx = ntx: tile ntx - 1 alone -- so a cell's four
// LUTs are constant and only the weights vary per pixel.  A page has cells_along(h, t) x cells_along(w, t) non-empty cells,
// at most (nty + 1) x (ntx + 1).
//
// Not supported: per-page or per-region settings; other colour models (the luma weights are fixed; an RGB8 page is all there is);
// enhancing in rt_resize_both, rt_det_preprocess or rt_crop_images, which take the page as it is.
// What is not claimed: that enhanced pages are read better.  The weights here are synthetic; the effect on recognition accuracy
// with trained PP-OCRv4 weights has not been measured.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include "geom_math.h"

namespace rt {
class Profiler;   // runtime.h
namespace pe {

constexpr int MIN_TILE = 32, MAX_TILE = 512, TILE_STEP = 32;

// nullptr when (tile, clip) is accepted, else what is wrong with it; tile = 0 is "off" whatever clip is
inline const char* check_params(int tile, float clip) {
  if (tile == 0) return nullptr;
  if (tile < MIN_TILE || tile > MAX_TILE || tile % TILE_STEP) return "tile must be 0 (off) or a multiple of 32 in [32, 512]";
  if (!(clip == clip)) return "clip is NaN";
  if (!(clip - clip == 0.0f)) return "clip is infinite";
  if (clip < 1.0f || clip > 64.0f) return "clip must be in [1, 64]";
  return nullptr;
}
inline int clip_x16_of(float clip) { return (int)lrintf(clip * 16.0f); }

RT_HD int luma(int r, int g, int b) { return (77 * r + 150 * g + 29 * b + 128) >> 8; }
RT_HD int tiles_along(int n, int t) { return (n + t - 1) / t; }
RT_HD int cells_along(int n, int t) { return (n - 1 + t / 2) / t + 1; }
RT_HD int clip_limit(int clip_x16, int area) { const int l = (clip_x16 * area) >> 12; return l > 1 ? l : 1; }
// what bin i gains from the redistribution of `excess`: excess / 256, and one more iff i = (k * 256) / r for a k < r = excess % 256
// (r < 256, so those bins are distinct and the only candidate is k = ceil(i r / 256))
RT_HD int bin_gain(int i, int excess) {
  const int r = excess & 255, k = (i * r + 255) >> 8;
  return (excess >> 8) + ((k < r && (k * 256) / r == i) ? 1 : 0);
}
RT_HD int lut_value(int c, int area) { return (int)(((uint32_t)c * 255u + (uint32_t)(area / 2)) / (uint32_t)area); }

// the two tiles and the weight of the second along one direction, for pixel coordinate x of n tiles
struct Axis { int i0, i1, w; };
RT_HD Axis axis(int x, int t, int n) {
  const int u = 2 * x + 1 - t;
  if (n == 1 || u <= 0) return Axis{0, 0, 0};
  const int i0 = u / (2 * t);
  if (i0 >= n - 1) return Axis{n - 1, n - 1, 0};
  return Axis{i0, i0 + 1, u - 2 * t * i0};
}
// the weight of pixel coordinate x inside a cell whose tiles are c (axis() of any of its pixels)
RT_HD int cell_weight(const Axis& c, int x, int t) { return c.i1 > c.i0 ? 2 * x + 1 - t - 2 * t * c.i0 : 0; }
RT_HD int blend(int t, int wx, int wy, int a00, int a01, int a10, int a11) {
  const uint32_t T2 = 2u * (uint32_t)t, ux = (uint32_t)wx, uy = (uint32_t)wy;
  const uint32_t top = (T2 - ux) * (uint32_t)a00 + ux * (uint32_t)a01, bot = (T2 - ux) * (uint32_t)a10 + ux * (uint32_t)a11;
  return (int)(((T2 - uy) * top + uy * bot + T2 * (uint32_t)t) / (T2 * T2));
}
RT_HD int shift_channel(int v, int d) { const int s = v + d; return s < 0 ? 0 : s > 255 ? 255 : s; }

// ---- the kernels' descriptors (page_enhance.hip): one per page of a lane part ----------------------------------------------
// src: the page (h x w RGB8, rows of 3 w bytes), dst: the enhanced page, luts: nty * ntx LUTs of 256 bytes (16-byte aligned).
// tile_base / cell_base: the page's first entry in the part's flat lists of tiles / cells (every page has at least one of each,
// so the bases strictly increase): entry g belongs to the last page whose base is <= g.
struct DevPage {
  const uint8_t* src; uint8_t* dst; uint8_t* luts;
  int h, w, nty, ntx, ncy, ncx;
  uint32_t tile_base, cell_base;
};
// fills the geometry and the bases of pages[0 .. n) from their h / w; returns false when a list would pass 2^31 - 1 entries
inline bool plan_pages(DevPage* pages, int n, int tile) {
  uint64_t tiles = 0, cells = 0;
  for (int i = 0; i < n; i++) {
    DevPage& p = pages[i];
    p.nty = tiles_along(p.h, tile); p.ntx = tiles_along(p.w, tile);
    p.ncy = cells_along(p.h, tile); p.ncx = cells_along(p.w, tile);
    p.tile_base = (uint32_t)tiles; p.cell_base = (uint32_t)cells;
    tiles += (uint64_t)p.nty * p.ntx; cells += (uint64_t)p.ncy * p.ncx;
    if (tiles > 0x7fffffffu || cells > 0x7fffffffu) return false;
  }
  return true;
}
#ifdef __HIPCC__
// both launches over pages[0 .. n) (d_pages: their copy on the device), on st: k_enhance_lut over the flat list of tiles, then
// k_enhance_apply over the flat list of cells; prof (or null): the launches' profile families page_enhance_lut / _apply
void launch(hipStream_t st, Profiler* prof, const DevPage* d_pages, const DevPage* pages, int n, int tile, int clip_x16);
#endif

// ---- the rule on the CPU, in plain loops ------------------------------------------------------------------------------------
// out [h * w * 3]; luts_out (or null) [nty * ntx * 256]
inline void enhance_page_host(const uint8_t* rgb, int h, int w, int tile, int clip_x16, uint8_t* out, uint8_t* luts_out) {
  const int nty = tiles_along(h, tile), ntx = tiles_along(w, tile);
  uint8_t* luts = luts_out ? luts_out : new uint8_t[(size_t)nty * ntx * 256];
  for (int ty = 0; ty < nty; ty++)
    for (int tx = 0; tx < ntx; tx++) {
      const int y0 = ty * tile, y1 = y0 + tile < h ? y0 + tile : h, x0 = tx * tile, x1 = x0 + tile < w ? x0 + tile : w;
      const int area = (y1 - y0) * (x1 - x0), L = clip_limit(clip_x16, area);
      int hist[256] = {}, excess = 0, c = 0;
      for (int y = y0; y < y1; y++)
        for (int x = x0; x < x1; x++) {
          const uint8_t* p = rgb + ((size_t)y * w + x) * 3;
          hist[luma(p[0], p[1], p[2])]++;
        }
      for (int i = 0; i < 256; i++)
        if (hist[i] > L) { excess += hist[i] - L; hist[i] = L; }
      uint8_t* lut = luts + ((size_t)ty * ntx + tx) * 256;
      for (int i = 0; i < 256; i++) { c += hist[i] + bin_gain(i, excess); lut[i] = (uint8_t)lut_value(c, area); }
    }
  for (int y = 0; y < h; y++) {
    const Axis ay = axis(y, tile, nty);
    for (int x = 0; x < w; x++) {
      const Axis ax = axis(x, tile, ntx);
      const uint8_t* p = rgb + ((size_t)y * w + x) * 3;
      uint8_t* o = out + ((size_t)y * w + x) * 3;
      const int Y = luma(p[0], p[1], p[2]);
      const uint8_t* r0 = luts + (size_t)ay.i0 * ntx * 256; const uint8_t* r1 = luts + (size_t)ay.i1 * ntx * 256;
      const int d = blend(tile, ax.w, ay.w, r0[ax.i0 * 256 + Y], r0[ax.i1 * 256 + Y], r1[ax.i0 * 256 + Y], r1[ax.i1 * 256 + Y]) - Y;
      for (int ch = 0; ch < 3; ch++) o[ch] = (uint8_t)shift_channel(p[ch], d);
    }
  }
  if (!luts_out) delete[] luts;
}

}  // namespace pe
}  // namespace rt
