// Page derule: the ruling lines of forms and tables -- table grids, underlines, the ______ of a blank field -- erased from a page
// before anything else reads it.  Written once for the gfx950 kernels (page_derule.hip), the CPU restatement (derule_page_host
// below: rt_debug_derule_page_host) and the session (derule_pages: session.cpp).  A rule that touches a row of text welds it to its
// neighbours in the DB probability map, and a rule inside a crop is read as _ | l or 1; callers remove lines on the host today
// (Leptonica's line removal is the well-known example), which takes the pages off the device.  The reference has no counterpart;
// the rule here is this project's own.  It is integer comparisons and copies of pixels only, so the kernels, the CPU restatement
// and a test's reference agree byte for byte.
//
// Setting.  rt_set_page_derule(s, min_len, max_thick, ink), per session.  min_len = 0: off, the initial state (the other two are
// then not looked at).  Otherwise 16 <= min_len <= 512 (pixels, any value), 1 <= max_thick <= 8 and 1 <= ink <= 255.  Anything
// else: RT_ERR_INVALID naming the parameter.
//
// The rule.  L = min_len, T = max_thick, I = ink.  One horizontal pass H(page) over an h x w RGB8 page:
//   1. Ink bits.  B[y][x] = (255 - pe::luma(r, g, b)) >= I (is_ink), the luma of page_enhance.h.
//   2. Runs.  hrun(y, x) = the length of the maximal horizontal run of B through the pixel, 0 where B is clear.  Every column falls
//      into maximal vertical runs [y0, y1] of B.
//   3. Removable run.  A vertical run is removable when y1 - y0 + 1 <= T, at least one of its pixels has hrun >= L, and it has a
//      fill (4): the thin cross-section of a long horizontal line.  A stroke that crosses the line has a longer vertical run and
//      stays, and so does a filled bar.
//   4. Fill.  The sources are a = (y0 - 2, x) when y0 >= 2 and b = (y1 + 2, x) when y1 + 2 <= h - 1, one pixel beyond the
//      anti-aliased fringe, both read from the pass's INPUT.  Neither exists (h <= T + 2 at most): the run has no fill and is left
//      as it is.  One exists: that one.  Both: the one with the larger luma, on a tie a (pick_b) -- the lighter is the likelier paper.
//   5. Output, per pixel (gather form).  A B pixel of a removable run takes the run's fill.  A clear pixel takes the fill of the
//      removable run that starts at y + 1; failing that, of the removable run that ends at y - 1 (the one-pixel fringe); failing
//      that too it keeps the input pixel, as every other pixel does.
// derule(page) = transpose(H(transpose(H(page)))): the vertical pass recomputes B from the horizontal pass's output.  That order
// removes grid junctions without a junction rule: after H a crossing is an ordinary piece of the vertical line.
// The output is always a new buffer; a caller's RT_MEM_DEVICE page is never written.  With flatten, enhance and deskew on as well
// the page is derule(deskew(enhance(flatten(page)))): lines must be level before their runs are long.  It moves no coordinate.
//
// What is not claimed.  A line steeper than about T / L breaks into runs shorter than L and stays.  Dashed and dotted rules stay.
// What derule does to recognition accuracy with trained PP-OCRv4 weights has not been measured (the weights here are synthetic).
// Not supported: per-page or per-region settings; derule in rt_resize_both, rt_det_preprocess or rt_crop_images; the removed
// segments as a table structure.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>
#include "geom_math.h"
#include "page_enhance.h"

namespace rt {
class Profiler;   // runtime.h
namespace pr {

constexpr int MIN_LEN = 16, MAX_LEN = 512, MAX_THICK = 8;

// nullptr when (min_len, max_thick, ink) is accepted, else what is wrong with it; min_len = 0 is "off" whatever the others are
inline const char* check_params(int min_len, int max_thick, int ink) {
  if (min_len == 0) return nullptr;
  if (min_len < MIN_LEN || min_len > MAX_LEN) return "min_len must be 0 (off) or in [16, 512]";
  if (max_thick < 1 || max_thick > MAX_THICK) return "max_thick must be in [1, 8]";
  if (ink < 1 || ink > 255) return "ink must be in [1, 255]";
  return nullptr;
}

RT_HD int luma_of(const uint8_t* p) { return pe::luma(p[0], p[1], p[2]); }
RT_HD bool is_ink(int r, int g, int b, int ink) { return 255 - pe::luma(r, g, b) >= ink; }
// whether the fill is source b, given which of the two exist (at least one) and their lumas
RT_HD bool pick_b(bool has_a, bool has_b, int luma_a, int luma_b) { return has_b && (!has_a || luma_b > luma_a); }

// ---- the kernels' descriptors (page_derule.hip): one per page of a lane part -----------------------------------------------
// src: the page (h x w RGB8, rows of 3 w bytes), mid: H(src), dst: the deruled page.  bits / keep / lng: bit-planes of h rows of
// wp = ceil(w / 32) words, bit x of a row in word x / 32 at position x % 32, the bits past w clear: B of the pass's input, the
// vertical pass's erosion, and the pixels of the pass's long runs.  The part's flat work lists: strips (4 rows x STRIP_PX pixels:
// k_derule_bits), row groups (4 rows, a wave each: k_derule_hlong), sweep blocks (256 lanes, each a word column of one segment of
// `seg` rows: k_derule_vsweep) and tiles (TILE_H x TILE_W pixels: k_derule_fill); *_base: the page's first entry in each.  Every
// page has at least one of each, so the bases strictly increase: entry g belongs to the last page whose base is <= g.
constexpr int STRIP_PX = 1024, STRIP_ROWS = 4, TILE_H = 32, TILE_W = 128, SWEEP_WG = 256, MAX_ROW_WORDS = 512;
struct DevPage {
  const uint8_t* src; uint8_t* mid; uint8_t* dst; uint32_t* bits; uint32_t* keep; uint32_t* lng;
  int h, w, wp, strips_x, nseg, tiles_y, tiles_x;
  uint32_t strip_base, group_base, sweep_base, tile_base;
};
// the rows of a vertical sweep's segment: a lane walks seg + min_len - 1 rows to write seg of them, so long segments waste less
// and short ones fill the chip; between 2 and 5 times the rows at either end of the range
RT_HD int sweep_seg(int min_len) { return min_len < 32 ? 32 : min_len > 128 ? 128 : min_len; }
// fills the geometry and the bases of pages[0 .. n) from their h / w.  Returns nullptr, or why the part cannot run: a row of more
// than MAX_ROW_WORDS words does not fit a wave's registers in k_derule_hlong's widest instance
inline const char* plan_pages(DevPage* pages, int n, int min_len) {
  uint64_t strips = 0, groups = 0, sweeps = 0, tiles = 0;
  const int seg = sweep_seg(min_len);
  for (int i = 0; i < n; i++) {
    DevPage& p = pages[i];
    p.wp = (p.w + 31) / 32;
    if (p.wp > MAX_ROW_WORDS) return "a page wider than 16384 pixels";
    if (p.h > 0x7fffffff - MAX_LEN - TILE_H) return "a page taller than 2^31 - 545 rows";
    const int g4 = (p.h + STRIP_ROWS - 1) / STRIP_ROWS;
    p.strips_x = (p.w + STRIP_PX - 1) / STRIP_PX;
    p.nseg = (p.h + seg - 1) / seg;
    p.tiles_y = (p.h + TILE_H - 1) / TILE_H; p.tiles_x = (p.w + TILE_W - 1) / TILE_W;
    p.strip_base = (uint32_t)strips; p.group_base = (uint32_t)groups; p.sweep_base = (uint32_t)sweeps; p.tile_base = (uint32_t)tiles;
    strips += (uint64_t)g4 * p.strips_x; groups += (uint64_t)g4;
    sweeps += ((uint64_t)p.nseg * p.wp + SWEEP_WG - 1) / SWEEP_WG; tiles += (uint64_t)p.tiles_y * p.tiles_x;
    if (strips > 0x7fffffffu || sweeps > 0x7fffffffu || tiles > 0x7fffffffu) return "more than 2^31 - 1 workgroups in one call";
  }
  return nullptr;
}
#ifdef __HIPCC__
// the seven launches over pages[0 .. n) (d_pages: their copy on the device), on st -- the horizontal pass: k_derule_bits, k_derule_hlong,
// k_derule_fill; the vertical pass: k_derule_bits, k_derule_vsweep twice (erode, dilate), k_derule_fill; prof (or null): the families
// page_derule_bits / _hlong / _vsweep / _fill
void launch(hipStream_t st, Profiler* prof, const DevPage* d_pages, const DevPage* pages, int n, int min_len, int max_thick, int ink);
#endif

// ---- the rule on the CPU, in plain loops ------------------------------------------------------------------------------------
// H(in) -> out, both [h * w * 3]
inline void hpass_host(const uint8_t* in, int h, int w, int L, int T, int I, uint8_t* out) {
  std::vector<uint8_t> B((size_t)h * w);
  std::vector<int> hrun((size_t)h * w, 0);
  for (int y = 0; y < h; y++) {
    for (int x = 0; x < w; x++) { const uint8_t* p = in + ((size_t)y * w + x) * 3; B[(size_t)y * w + x] = is_ink(p[0], p[1], p[2], I); }
    for (int x = 0; x < w;) {
      if (!B[(size_t)y * w + x]) { x++; continue; }
      int x1 = x;
      while (x1 + 1 < w && B[(size_t)y * w + x1 + 1]) x1++;
      for (int i = x; i <= x1; i++) hrun[(size_t)y * w + i] = x1 - x + 1;
      x = x1 + 1;
    }
  }
  memcpy(out, in, (size_t)h * w * 3);
  // Runs from the top down: a run's upper fringe pixel overwrites what the run above it left there (the run that starts at y + 1
  // comes first in 5), and its lower fringe pixel is overwritten by the next run for the same reason.
  for (int x = 0; x < w; x++)
    for (int y = 0; y < h;) {
      if (!B[(size_t)y * w + x]) { y++; continue; }
      const int y0 = y;
      bool lng = false;
      for (; y < h && B[(size_t)y * w + x]; y++) lng = lng || hrun[(size_t)y * w + x] >= L;
      const int y1 = y - 1;
      const bool has_a = y0 >= 2, has_b = y1 + 2 <= h - 1;
      if (y1 - y0 + 1 > T || !lng || (!has_a && !has_b)) continue;
      const uint8_t* a = in + ((size_t)(has_a ? y0 - 2 : 0) * w + x) * 3;
      const uint8_t* b = in + ((size_t)(has_b ? y1 + 2 : 0) * w + x) * 3;
      const uint8_t* f = pick_b(has_a, has_b, luma_of(a), luma_of(b)) ? b : a;
      for (int yy = (y0 > 0 ? y0 - 1 : 0); yy <= (y1 + 1 < h ? y1 + 1 : h - 1); yy++) memcpy(out + ((size_t)yy * w + x) * 3, f, 3);
    }
}
inline void transpose_host(const uint8_t* in, int h, int w, uint8_t* out) {   // out [w][h]
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) memcpy(out + ((size_t)x * h + y) * 3, in + ((size_t)y * w + x) * 3, 3);
}
// out [h * w * 3]
inline void derule_page_host(const uint8_t* rgb, int h, int w, int min_len, int max_thick, int ink, uint8_t* out) {
  std::vector<uint8_t> a((size_t)h * w * 3), b((size_t)h * w * 3);
  hpass_host(rgb, h, w, min_len, max_thick, ink, a.data());
  transpose_host(a.data(), h, w, b.data());
  hpass_host(b.data(), w, h, min_len, max_thick, ink, a.data());
  transpose_host(a.data(), w, h, out);
}

}  // namespace pr
}  // namespace rt
