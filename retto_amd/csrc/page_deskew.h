// Page deskew: the skew of a page estimated from its own text lines and the page rotated back by it, before anything else reads the
// page.  Written once for the gfx950 kernels (page_deskew.hip), the CPU restatement (deskew_page_host below:
// rt_debug_deskew_page_host) and the session (deskew_pages: session.cpp).  Page flatten and page enhance correct a page's light and
// contrast; nothing corrected its geometry: a scan or photograph a few degrees off gives slanted DB quads, a rotating warp per line
// crop, and a reading order, word boxes and keyword quads that inherit the slant.  Leptonica, Tesseract and the scanner apps all
// straighten the page first; here it is the third page filter, deskew(enhance(flatten(page))).  The reference has no counterpart;
// the rule here is this project's own.  All arithmetic is 32-bit and 64-bit integer -- no tan, cos or sqrt of a maths library
// anywhere -- so the kernels, the CPU restatement and a test's reference agree byte for byte.
//
// Setting.  rt_set_page_deskew(s, range, min_gain), per session.  range = 0: off, the initial state (min_gain is then not looked
// at).  Otherwise 1 <= range <= 128 and 0 <= min_gain <= 10000.  Anything else: RT_ERR_INVALID naming the parameter.
//
// The rule, for a page of h x w RGB8 pixels, K = range, G = min_gain; the unit of slope is 1 / 512 (about 0.112 degrees):
//   1. Cells.  c = 4, doubled while ceil(max(h, w) / c) > 512 (cell_size); gh = ceil(h / c), gw = ceil(w / c);
//      I[gy][gx] = 255 - the minimum of pe::luma over the cell's pixels.  Edge cells are partial, nothing is padded.
//   2. Profiles.  For k in [-K, K]: d_k(gx) = ((gx - gw / 2) * k * 128 + 32768) >> 16, an arithmetic shift (shift_of);
//      P_k[r] = the sum of I[gy][gx] over all cells with gy + d_k(gx) = r; S_k = the sum over r of (P_k[r + 1] - P_k[r])^2, from
//      below the first non-zero row to above the last, the two zero ends included, in uint64.  |d_k| <= max_shift(gw, K) <= 64,
//      so there are at most 640 rows that can be non-zero; |P| <= 512 * 255 and S < 2^44.
//   3. Choice.  k* = the k of largest S_k; ties go to the smaller |k|, then to the positive one (better).  If
//      S_k* * 100 < S_0 * (100 + G) then k* = 0 (gated).  A small grid cannot tell small slopes from none: every d_k is 0 there,
//      the S_k are equal, and the tie rule makes that case 0.  Positive k: the lines rise to the right.
//   4. Angle.  a = |k*|, q = 512^2 + a^2, r = isqrt(q << 16) (the floor square root); cosq = (512 * 2^24 + r / 2) / r,
//      sinq = sign(k*) * ((a * 2^24 + r / 2) / r), in 64-bit: cosine and sine in units of 2^-16 (angle_of).  The 129 pairs are a
//      table built on the host by this rule and uploaded once per session; the kernels index it.
//   5. Turn.  k* = 0: the output is a copy of the source.  Otherwise for output pixel (x, y): dx = 2 x - (w - 1), dy = 2 y - (h - 1),
//      U = cosq dx + sinq dy + (w - 1) 65536, V = -sinq dx + cosq dy + (h - 1) 65536 (units of 2^-17 pixel, 64-bit);
//      u0 = U >> 17, fu = (U >> 9) & 255, v0 and fv likewise; the four sample coordinates u0, u0 + 1, v0, v0 + 1 are clamped to the
//      page (edge replicate) (sample_at); per channel
//      out = ((256 - fu)(256 - fv) p00 + fu (256 - fv) p01 + (256 - fu) fv p10 + fu fv p11 + 32768) >> 16 (blend).
//   6. The matrix of rt_results_page_deskew, a point (x, y) of the deskewed page to (u, v) of the original: cs = cosq / 65536,
//      sn = sinq / 65536, cx = (w - 1) / 2, cy = (h - 1) / 2; u = cx + cs (x - cx) + sn (y - cy), v = cy - sn (x - cx) + cs (y - cy)
//      (matrix_of; the identity for k* = 0).
// The output has the size of the input and is always a new buffer; a caller's RT_MEM_DEVICE page is never written.  Every box,
// word box and keyword quad of a deskewed call is in the DESKEWED page's coordinates; rt_results_page_deskew returns the map back.
//
// Not supported: per-page settings; deskew in rt_run_regions* (the caller's quads define the geometry there) or in the stage
// functions; mapping the results back to the original page; slopes beyond 128 / 512 (14 degrees); upside-down or sideways pages.
// What is not claimed: that deskewed pages are read better.  The weights here are synthetic; the effect on recognition accuracy
// with trained PP-OCRv4 weights has not been measured.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>
#include "geom_math.h"
#include "page_enhance.h"

namespace rt {
class Profiler;   // runtime.h
namespace pd {

constexpr int MAX_RANGE = 128, MAX_GAIN = 10000, MAX_GRID = 512;

// nullptr when (range, min_gain) is accepted, else what is wrong with it; range = 0 is "off" whatever min_gain is
inline const char* check_params(int range, int min_gain) {
  if (range == 0) return nullptr;
  if (range < 1 || range > MAX_RANGE) return "range must be 0 (off) or in [1, 128]";
  if (min_gain < 0 || min_gain > MAX_GAIN) return "min_gain must be in [0, 10000]";
  return nullptr;
}

RT_HD int cell_size(int h, int w) {
  const int m = h > w ? h : w;
  int c = 4;
  while ((m - 1) / c + 1 > MAX_GRID) c *= 2;
  return c;
}
RT_HD int cells_along(int n, int c) { return (n - 1) / c + 1; }
RT_HD int shift_of(int gx, int gw, int k) { return ((gx - gw / 2) * k * 128 + 32768) >> 16; }
// the largest |d_k(gx)| over |k| <= K and the columns of a grid gw wide (|gx - gw / 2| <= gw / 2; a negative product rounds no further out)
RT_HD int max_shift(int gw, int K) { return ((gw / 2) * K * 128 + 32768) >> 16; }
// (s, k) before (sb, kb) in the order of step 3
RT_HD bool better(uint64_t s, int k, uint64_t sb, int kb) {
  if (s != sb) return s > sb;
  const int a = k < 0 ? -k : k, ab = kb < 0 ? -kb : kb;
  return a != ab ? a < ab : k > kb;
}
RT_HD bool gated(uint64_t s_best, uint64_t s0, int min_gain) { return s_best * 100u < s0 * (uint64_t)(100 + min_gain); }

// the record k_deskew_pick leaves per page: the chosen slope and its (cosq, sinq), (65536, 0) for 0
struct Record { int32_t k, cosq, sinq; };
inline uint64_t isqrt64(uint64_t v) {
  uint64_t r = 0;
  for (uint64_t b = 1ull << 62; b; b >>= 2) {
    if (v >= r + b) { v -= r + b; r = (r >> 1) + b; } else r >>= 1;
  }
  return r;
}
inline Record angle_of(int k) {
  const uint64_t a = (uint64_t)(k < 0 ? -k : k), r = isqrt64((512ull * 512ull + a * a) << 16);
  const int32_t s = (int32_t)(((a << 24) + r / 2) / r);
  return Record{k, (int32_t)(((512ull << 24) + r / 2) / r), k < 0 ? -s : s};
}
// the table of step 4: (cosq, sinq) of a = 0 .. 128, [129][2]
inline std::vector<int32_t> angle_table() {
  std::vector<int32_t> t(2 * (MAX_RANGE + 1));
  for (int a = 0; a <= MAX_RANGE; a++) { const Record r = angle_of(a); t[2 * a] = r.cosq; t[2 * a + 1] = r.sinq; }
  return t;
}
inline void matrix_of(const Record& r, int h, int w, float m[6]) {
  const double cs = r.cosq / 65536.0, sn = r.sinq / 65536.0, cx = (w - 1) / 2.0, cy = (h - 1) / 2.0;
  m[0] = (float)cs; m[1] = (float)sn; m[2] = (float)(cx - cs * cx - sn * cy);
  m[3] = (float)-sn; m[4] = (float)cs; m[5] = (float)(cy + sn * cx - cs * cy);
}

// step 5: where output pixel (x, y) samples the source and with which weights
struct Sample { int x0, x1, y0, y1, fu, fv; };
RT_HD int clampi(long long v, int hi) { return v < 0 ? 0 : v > hi ? hi : (int)v; }
RT_HD long long turn_u(int x, int y, int h, int w, int cosq, int sinq) {
  return (long long)cosq * (2 * x - (w - 1)) + (long long)sinq * (2 * y - (h - 1)) + (long long)(w - 1) * 65536;
}
RT_HD long long turn_v(int x, int y, int h, int w, int cosq, int sinq) {
  return -(long long)sinq * (2 * x - (w - 1)) + (long long)cosq * (2 * y - (h - 1)) + (long long)(h - 1) * 65536;
}
RT_HD Sample sample_at(int x, int y, int h, int w, int cosq, int sinq) {
  const long long U = turn_u(x, y, h, w, cosq, sinq), V = turn_v(x, y, h, w, cosq, sinq);
  const long long u0 = U >> 17, v0 = V >> 17;
  return Sample{clampi(u0, w - 1), clampi(u0 + 1, w - 1), clampi(v0, h - 1), clampi(v0 + 1, h - 1), (int)((U >> 9) & 255), (int)((V >> 9) & 255)};
}
RT_HD int blend(int fu, int fv, int p00, int p01, int p10, int p11) {
  return ((256 - fu) * (256 - fv) * p00 + fu * (256 - fv) * p01 + (256 - fu) * fv * p10 + fu * fv * p11 + 32768) >> 16;
}

// ---- the kernels' descriptors (page_deskew.hip): one per page of a lane part ----------------------------------------------
// src: the page (h x w RGB8, rows of 3 w bytes), dst: the deskewed page; cells: I transposed, [gw] columns of gp bytes, gp = gh
// rounded up to a dword so that k_deskew_profile stages whole columns with dword loads; scores: S_k, [2 K + 1]; rec: the page's
// record.  A cells strip is one row of cells cut into pieces of cells_per_strip cells (STRIP_PX pixels, or one cell where a cell is
// wider: it is then walked in `pieces` pieces of STRIP_PX pixels); strip_base / tile_base: the page's first entry in the part's
// flat lists of strips and of rotate tiles (TILE x TILE pixels).  Every page has at least one of each, so the bases strictly
// increase: entry g belongs to the last page whose base is <= g.  k_deskew_profile takes ANGLES_PER_WG candidate angles of one
// page per workgroup, page-major.
constexpr int STRIP_PX = 1024, TILE = 32, ANGLES_PER_WG = 8;
struct DevPage {
  const uint8_t* src; uint8_t* dst; uint8_t* cells; uint64_t* scores; Record* rec;
  int h, w, c, gh, gw, gp, cells_per_strip, pieces, strips_x, tiles_y, tiles_x;
  uint32_t strip_base, tile_base;
};
inline int angle_blocks(int K) { return (2 * K + 1 + ANGLES_PER_WG - 1) / ANGLES_PER_WG; }
// fills the geometry and the bases of pages[0 .. n) from their h / w; returns false when a list would pass 2^31 - 1 entries
inline bool plan_pages(DevPage* pages, int n, int K) {
  uint64_t strips = 0, tiles = 0;
  for (int i = 0; i < n; i++) {
    DevPage& p = pages[i];
    p.c = cell_size(p.h, p.w); p.gh = cells_along(p.h, p.c); p.gw = cells_along(p.w, p.c); p.gp = (p.gh + 3) & ~3;
    p.cells_per_strip = p.c >= STRIP_PX ? 1 : STRIP_PX / p.c; p.pieces = p.c > STRIP_PX ? p.c / STRIP_PX : 1;
    p.strips_x = (p.gw + p.cells_per_strip - 1) / p.cells_per_strip;
    p.tiles_y = (p.h + TILE - 1) / TILE; p.tiles_x = (p.w + TILE - 1) / TILE;
    p.strip_base = (uint32_t)strips; p.tile_base = (uint32_t)tiles;
    strips += (uint64_t)p.gh * p.strips_x; tiles += (uint64_t)p.tiles_y * p.tiles_x;
    if (strips > 0x7fffffffu || tiles > 0x7fffffffu) return false;
  }
  return (uint64_t)n * (uint64_t)angle_blocks(K) <= 0x7fffffffu;
}
#ifdef __HIPCC__
// the four launches over pages[0 .. n) (d_pages: their copy on the device), on st: k_deskew_cells over the flat list of strips,
// k_deskew_profile over pages x blocks of angles, k_deskew_pick over the pages, k_deskew_rotate over the tiles; d_table: the
// angle table on the device; prof (or null): the families page_deskew_cells / _profile / _pick / _rotate
void launch(hipStream_t st, Profiler* prof, const DevPage* d_pages, const DevPage* pages, int n, int K, int min_gain, const int32_t* d_table);
#endif

// ---- the rule on the CPU, in plain loops ------------------------------------------------------------------------------------
// out [h * w * 3]; slope: k*; scores_out (or null) [2 K + 1]: S_k
inline void deskew_page_host(const uint8_t* rgb, int h, int w, int K, int min_gain, uint8_t* out, int* slope, uint64_t* scores_out) {
  const int c = cell_size(h, w), gh = cells_along(h, c), gw = cells_along(w, c), D = max_shift(gw, K);
  std::vector<int> I((size_t)gh * gw);
  for (int gy = 0; gy < gh; gy++)
    for (int gx = 0; gx < gw; gx++) {
      int m = 255;
      for (int y = c * gy; y < h && y < c * gy + c; y++)
        for (int x = c * gx; x < w && x < c * gx + c; x++) {
          const uint8_t* p = rgb + ((size_t)y * w + x) * 3;
          const int Y = pe::luma(p[0], p[1], p[2]);
          if (Y < m) m = Y;
        }
      I[(size_t)gy * gw + gx] = 255 - m;
    }
  std::vector<uint64_t> S((size_t)2 * K + 1);
  std::vector<long long> P((size_t)gh + 2 * D + 2);   // row r at P[r + D + 1]: a zero row at either end
  for (int k = -K; k <= K; k++) {
    std::fill(P.begin(), P.end(), 0);
    for (int gx = 0; gx < gw; gx++) {
      const int d = shift_of(gx, gw, k);
      for (int gy = 0; gy < gh; gy++) P[(size_t)(gy + d + D + 1)] += I[(size_t)gy * gw + gx];
    }
    uint64_t s = 0;
    for (size_t r = 0; r + 1 < P.size(); r++) { const long long df = P[r + 1] - P[r]; s += (uint64_t)(df * df); }
    S[(size_t)(k + K)] = s;
  }
  int best = 0;
  for (int k = -K; k <= K; k++) if (better(S[(size_t)(k + K)], k, S[(size_t)(best + K)], best)) best = k;
  if (gated(S[(size_t)(best + K)], S[(size_t)K], min_gain)) best = 0;
  if (scores_out) memcpy(scores_out, S.data(), S.size() * sizeof(uint64_t));
  *slope = best;
  if (best == 0) { memcpy(out, rgb, (size_t)h * w * 3); return; }
  const Record r = angle_of(best);
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      const Sample s = sample_at(x, y, h, w, r.cosq, r.sinq);
      const uint8_t* p00 = rgb + ((size_t)s.y0 * w + s.x0) * 3; const uint8_t* p01 = rgb + ((size_t)s.y0 * w + s.x1) * 3;
      const uint8_t* p10 = rgb + ((size_t)s.y1 * w + s.x0) * 3; const uint8_t* p11 = rgb + ((size_t)s.y1 * w + s.x1) * 3;
      for (int ch = 0; ch < 3; ch++) out[((size_t)y * w + x) * 3 + ch] = (uint8_t)blend(s.fu, s.fv, p00[ch], p01[ch], p10[ch], p11[ch]);
    }
}

}  // namespace pd
}  // namespace rt
