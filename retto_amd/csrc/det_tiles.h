// Det tiles: the detector run over overlapping tiles of a large page, written once for the session (det_groups: session.cpp), the
// two data-movement kernels (k_det_tile_cut, k_det_tile_stitch: prepost_kernels.hip), rt_det_tile_plan and the CPU check
// (tests/native/det_tiles_driver.cpp).  A page whose det input is far larger than anything the det network was trained or tuned
// at -- a 7680 x 4320 scan detected at its own resolution -- is cut into tiles of one fixed size; the network runs on the tiles,
// and each tile's trusted part is written into the ONE page probability map that DB post-processing reads.  Nothing downstream
// changes: no boxes are merged, the geometry is the page's.  The reference has no counterpart (PaddleOCR's sliced inference
// merges boxes instead); the rule here is this project's own.  This header needs no HIP header, so a stand-alone program can
// include it.
//
// The plan along one axis.  A det input of H x W has both dimensions a multiple of 32 (gm::resize_either_dims).  For tile T and
// overlap O the plan along an axis of length L is
//   L <= T     one tile [0, L);
//   otherwise  n = ceil((L - T) / (T - O)) + 1 tiles of length T at origins x_i = min(i (T - O), L - T): every tile is full
//              size, and only the last pair may overlap by more than O.
// Ownership.  b_-1 = 0, b_i = (x_i + T + x_{i+1}) / 2 for i < n - 1 (the middle of the pair's overlap), b_{n-1} = L; pixel x
// belongs to the one tile i with b_{i-1} <= x < b_i.  All x_i, T and L are multiples of 32, so every b_i is a multiple of 16: a
// 4-float store never straddles an ownership boundary.  An interior boundary lies at least O / 2 inside both tiles of its pair:
// the outer half of a tile's overlap, where its zero padding and truncated text act, is discarded.
// A page's tiles are the product of its row plan and its column plan, in row-major order, and
//   page_map[y][x] = tile_map(ty(y), tx(x))[y - y0][x - x0],
// a pure selection: the stitch is exact, every page pixel is written once, and the order of the tiles does not matter.
// A page with H <= T and W <= T is not tiled: it takes the whole-page path bit for bit.
//
// Parameters.  T = 0 is off.  Otherwise T is a multiple of 32 with T >= MIN_TILE, O a multiple of 32 with 0 <= O <= T / 2 (so
// the stride T - O is at least T / 2 and interior tiles own at least T - O pixels).  check_params() names the parameter.
//
// The largest det input.  DB post-processing (dbpost_kernels.hip) indexes a page's pixels, rows and hull points with int: the
// pixel index H * W, row_cap = 3 H W + 1024 and hull_cap = 2 row_cap + 4 contour_cap = 8 H W + 6144 (carve()).  The last is the
// first to pass 2^31 - 1, at H W = 268 434 687; MAX_DET_PIXELS is that rounded down to whole 32 x 32 cells.  Its workspace takes
// about 120 bytes per pixel (db_workspace_bytes), 4 GB for a 7680 x 4320 page.  A page beyond the limit fails with ERR_CAPACITY
// before anything is queued, tiled or not.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define RT_DT_HD __host__ __device__
#else
#define RT_DT_HD
#endif

namespace rt {
namespace dt {

constexpr int OK = 0, ERR_INVALID = 8, ERR_CAPACITY = 9;   // rt_status values
constexpr int CELL = 32;         // what every det dimension, tile and overlap is a multiple of
constexpr int MIN_TILE = 64;
constexpr long long MAX_DET_PIXELS = 268434432;   // (2^28 - 1024): see "The largest det input" above

// nullptr when (tile, overlap) is accepted, else what is wrong with which parameter
inline const char* check_params(int tile, int overlap) {
  if (tile < 0) return "tile is negative";
  if (tile == 0) return overlap < 0 ? "overlap is negative" : nullptr;   // off: the overlap is kept and not read
  if (tile % CELL != 0) return "tile must be 0 (off) or a multiple of 32";
  if (tile < MIN_TILE) return "tile must be 0 (off) or at least 64";
  if (overlap < 0) return "overlap is negative";
  if (overlap % CELL != 0) return "overlap must be a multiple of 32";
  if (overlap > tile / 2) return "overlap must be at most tile / 2";
  return nullptr;
}

// tiles along an axis of length L (T = 0: off)
RT_DT_HD inline int axis_tiles(int L, int T, int O) {
  if (T <= 0 || L <= T) return 1;
  const int stride = T - O;
  return (L - T + stride - 1) / stride + 1;
}
// length of every tile of the axis
RT_DT_HD inline int axis_tile_len(int L, int T) { return T <= 0 || L <= T ? L : T; }
// x_i, 0 <= i < axis_tiles
RT_DT_HD inline int axis_origin(int L, int T, int O, int i) {
  if (T <= 0 || L <= T) return 0;
  const long long x = (long long)i * (T - O);
  return x < L - T ? (int)x : L - T;
}
// b_i, -1 <= i < axis_tiles
RT_DT_HD inline int axis_bound(int L, int T, int O, int i) {
  if (i < 0) return 0;
  if (i >= axis_tiles(L, T, O) - 1) return L;
  return (axis_origin(L, T, O, i) + T + axis_origin(L, T, O, i + 1)) / 2;
}

// a page is tiled when tiles are on and it does not fit into one
RT_DT_HD inline bool page_tiled(int H, int W, int T) { return T > 0 && (H > T || W > T); }

struct Axis {
  int len = 0;                      // every tile's length
  std::vector<int> origin, bound;   // [n] each; tile i owns [i ? bound[i - 1] : 0, bound[i])
  int n() const { return (int)origin.size(); }
  int own0(int i) const { return i ? bound[(size_t)i - 1] : 0; }
};
inline Axis axis_plan(int L, int T, int O) {
  Axis a;
  a.len = axis_tile_len(L, T);
  const int n = axis_tiles(L, T, O);
  a.origin.resize((size_t)n); a.bound.resize((size_t)n);
  for (int i = 0; i < n; i++) { a.origin[(size_t)i] = axis_origin(L, T, O, i); a.bound[(size_t)i] = axis_bound(L, T, O, i); }
  return a;
}

// What a det input of H x W must satisfy whatever the tiles: OK, or ERR_INVALID / ERR_CAPACITY with *why set
inline int check_page(int H, int W, std::string* why) {
  if (H <= 0 || W <= 0 || H % CELL != 0 || W % CELL != 0) {
    if (why) *why = "a det input has positive dimensions that are multiples of 32, not " + std::to_string(H) + " x " + std::to_string(W);
    return ERR_INVALID;
  }
  if ((long long)H * W > MAX_DET_PIXELS) {
    if (why) *why = "a det input of " + std::to_string(H) + " x " + std::to_string(W) + " pixels is beyond the " +
                    std::to_string(MAX_DET_PIXELS) + " that DB post-processing indexes (lower max_side_len or the det limit)";
    return ERR_CAPACITY;
  }
  return OK;
}

// One tile of a launch group as the two kernels read it.  cut: rows [y0, y0 + th) x columns [x0, x0 + tw) of the page's RGB8 det
// image (page_w pixels a row) -> th x tw pixels, contiguous, at cut + cut_off.  stitch: the owned rectangle [oy0, oy1) x
// [ox0, ox1) of the tile's map at maps + map_off (tw floats a row) -> the same page coordinates of page_map.
struct TileDesc {
  const uint8_t* src;
  float* page_map;
  long long cut_off;   // bytes, a multiple of 256
  long long map_off;   // floats, a multiple of 1024
  int page_w, y0, x0, th, tw, oy0, oy1, ox0, ox1, pad_;
};

}  // namespace dt
}  // namespace rt
