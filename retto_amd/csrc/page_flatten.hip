// Page flatten on gfx950 (rt_set_page_flatten; page_flatten.h states the rule and holds every formula used here): the pages of one
// lane part in three launches, without global atomics and without synchronisation between workgroups.
//   k_flatten_pool   one workgroup of 256 lanes per strip (4 page rows x 1024 pixels) of the part's flat strip list: the strip's
//                    bytes go once through LDS -- a row segment is cut at its first aligned dword, the body moves as dwords, head
//                    and tail as bytes, each row at the LDS offset of its own misalignment so that global and LDS dwords coincide
//                    -- and a lane takes the maximum of one cell per channel from twelve aligned LDS dwords (the row's
//                    misalignment shifted out across dword pairs).  Bytes the strip does not have are zero, the identity of max.
//   k_flatten_level  one workgroup of 128 lanes per 32 x 32-cell tile and channel of the flat tile list: the tile and its halo of
//                    3 r cells (what lies inside the grid of it) staged in LDS as bytes with dword loads, then the six separable
//                    passes in LDS -- max along x, along y, min along x, along y (van Herk / Gil-Werman: suffix extrema of blocks
//                    of 2 r + 1 in a second buffer, prefix extrema in a register, two reads and two writes per cell whatever r
//                    is), box sum along x (running sum) and along y (prefix sums) -- and B written for the tile.  A lane owns a
//                    line of a pass.  Every window is clipped by the bounds of the grid inside the staged region: no cell outside
//                    the grid is ever read or stands in for anything.  After each pair of passes the outer r cells of the region
//                    hold values of windows cut by the region, not the grid; the next pair leaves them out, and after three
//                    pairs the tile is what remains.  The halo is recomputed per tile (at r = 16 the region is 16 times the
//                    tile), accepted because the grid is 1 / 16 of the page.
//   k_flatten_apply  one workgroup of 256 lanes per 32 x 128-pixel block of the flat block list: the 10 x 34 cells of B around
//                    the block (indices clamped to the grid, which is what axis() does at the border) in LDS, the three channels
//                    packed in a dword; a lane takes 4 pixels per step (rows cut by the destination address: page_rows.h), blends
//                    the level from four LDS dwords and divides with a float reciprocal corrected by the remainder
//                    (flat_value_rcp), into the new page.
// Every loop is bounded by the descriptors; every address is formed from coordinates clipped to the page or the grid.
#include "common.h"
#include "page_flatten.h"
#include "page_rows.h"
#include "runtime.h"

namespace rt {
namespace pf {
namespace {

using namespace rows;

constexpr int WG = 256, LEVEL_WG = 128;
constexpr int POOL_ROW_DW = 3 * POOL_CELLS + 4;                  // a strip row in LDS: 3072 bytes, up to 3 of misalignment, a spare dword
constexpr int REGION = TILE + 6 * MAX_RADIUS;                    // 128: the widest staged region
constexpr int PITCH = 140, PITCH_DW = PITCH / 4;                 // bytes per region row: 35 dwords, odd, so lanes on rows hit 64 banks
constexpr int APPLY_CY = APPLY_H / CELL + 2, APPLY_CX = APPLY_W / CELL + 2;
static_assert(REGION + 7 + 3 <= PITCH && (PITCH_DW & 1) && POOL_CELLS == WG, "LDS layouts");
static_assert((TILE + 2 * MAX_RADIUS) * TILE * 6 <= REGION * PITCH, "the sums reuse the second buffer");

enum { BY_STRIP, BY_TILE, BY_BLOCK };
// the last page whose strip_base / tile_base / block_base is <= g
__device__ inline int find_page(const DevPage* pages, int n, uint32_t g, int by) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    const uint32_t b = by == BY_STRIP ? pages[mid].strip_base : by == BY_TILE ? pages[mid].tile_base : pages[mid].block_base;
    if (b <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(WG) void k_flatten_pool(const DevPage* __restrict__ pages, int npages) {
  __shared__ uint32_t row[CELL][POOL_ROW_DW];
  const int t = threadIdx.x;
  const DevPage P = pages[find_page(pages, npages, blockIdx.x, BY_STRIP)];
  const uint32_t k = blockIdx.x - P.strip_base;
  if (k >= (uint32_t)P.gh * (uint32_t)P.strips_x) return;
  const int gy = (int)(k / (uint32_t)P.strips_x), sx = (int)(k - (uint32_t)gy * (uint32_t)P.strips_x);
  const int x0 = sx * POOL_CELLS * CELL, npx = min(P.w - x0, POOL_CELLS * CELL), nb = 3 * npx;
  for (int i = t; i < CELL * POOL_ROW_DW; i += WG) (&row[0][0])[i] = 0u;
  __syncthreads();
  int pad[CELL];
  for (int r = 0; r < CELL; r++) {
    const int y = CELL * gy + r;
    pad[r] = 0;
    if (y >= P.h) continue;                                        // (a partial cell row: the missing rows stay zero)
    const uint8_t* a = P.src + ((size_t)y * P.w + x0) * 3;
    pad[r] = (int)((uintptr_t)a & 3);
    const int head = min(nb, (4 - pad[r]) & 3), body = (nb - head) >> 2, tail = nb - head - 4 * body;
    uint8_t* l = (uint8_t*)row[r] + pad[r];                        // segment byte i at l[i]: l + head is a dword where a + head is
    if (t < head) l[t] = a[t];
    if (t < tail) l[head + 4 * body + t] = a[head + 4 * body + t];
    const uint32_t* g = (const uint32_t*)(a + head);
    uint32_t* ld = (uint32_t*)(l + head);
    for (int d = t; d < body; d += WG) ld[d] = g[d];
  }
  __syncthreads();
  const int gx = sx * POOL_CELLS + t;
  if (gx >= P.gw) return;
  uint32_t m0 = 0, m1 = 0, m2 = 0;                                  // R, G, B
  for (int r = 0; r < CELL; r++) {
    const uint32_t* q = &row[r][3 * t];
    const uint32_t q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    const int sh = 8 * pad[r];
    const uint32_t w0 = (uint32_t)((((uint64_t)q1 << 32) | q0) >> sh), w1 = (uint32_t)((((uint64_t)q2 << 32) | q1) >> sh),
                   w2 = (uint32_t)((((uint64_t)q3 << 32) | q2) >> sh);   // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
    m0 = max(max(m0, w0 & 255u), max(max(w0 >> 24, (w1 >> 16) & 255u), (w2 >> 8) & 255u));
    m1 = max(max(m1, (w0 >> 8) & 255u), max(max(w1 & 255u, w1 >> 24), (w2 >> 16) & 255u));
    m2 = max(max(m2, (w0 >> 16) & 255u), max(max((w1 >> 8) & 255u, w2 & 255u), w2 >> 24));
  }
  const size_t plane = (size_t)P.gh * P.gp, at = (size_t)gy * P.gp + gx;
  P.cells[at] = (uint8_t)m0; P.cells[plane + at] = (uint8_t)m1; P.cells[2 * plane + at] = (uint8_t)m2;
}

// One running-extremum pass in place: for the lines l0 <= l < l1 (a lane each), element i of line l at a[l * ls + i * es],
// a[i] = max or min of a over [max(lo, i - r), min(hi - 1, i + r)] for lo <= i < hi.  h: the second buffer, same layout.
// Blocks of k = 2 r + 1 elements counted from lo; the backward sweep leaves in h the extremum from each element to the end of its
// block (the last block ends at hi - 1), the forward sweep carries the extremum g from the start of the block of `right` to
// `right` and pr, the position of `right` in its block.  A window spans at most two blocks: h[left] and g together; inside one
// block it starts the block (g alone) or is cut at hi - 1 (h[left] alone).  Element i is written at step i + r, after it was read.
template <bool MAX>
__device__ inline void pass_extrema(uint8_t* a, uint8_t* h, int ls, int es, int l0, int l1, int lo, int hi, int r, int t) {
  const int k = 2 * r + 1;
  if (hi <= lo) return;
  for (int l = l0 + t; l < l1; l += LEVEL_WG) {
    uint8_t* al = a + l * ls; uint8_t* hl = h + l * ls;
    int m = 0, cnt = (hi - 1 - lo) % k;
    #pragma unroll 4
    for (int i = hi - 1; i >= lo; i--) {
      const int v = al[i * es];
      m = (i == hi - 1 || cnt == k - 1) ? v : MAX ? max(m, v) : min(m, v);
      hl[i * es] = (uint8_t)m;
      cnt = cnt == 0 ? k - 1 : cnt - 1;
    }
    int g = 0, pr = -1;
    #pragma unroll 4
    for (int j = lo; j < hi + r; j++) {
      if (j < hi) {
        const int v = al[j * es];
        pr = pr + 1 == k ? 0 : pr + 1;
        g = pr == 0 ? v : MAX ? max(g, v) : min(g, v);
      }
      const int i = j - r;
      if (i < lo) continue;
      const int left = max(lo, i - r), right = min(hi - 1, j), bs = right - pr;
      const int s = hl[left * es];
      al[i * es] = (uint8_t)(left == bs ? g : left > bs ? s : MAX ? max(s, g) : min(s, g));
    }
  }
}

__global__ __launch_bounds__(LEVEL_WG) void k_flatten_level(const DevPage* __restrict__ pages, int npages, int r) {
  __shared__ uint32_t buf_a[REGION * PITCH_DW], buf_h[REGION * PITCH_DW];
  const int t = threadIdx.x;
  const DevPage P = pages[find_page(pages, npages, blockIdx.x, BY_TILE)];
  uint32_t k = blockIdx.x - P.tile_base;
  const uint32_t per_ch = (uint32_t)P.tiles_y * (uint32_t)P.tiles_x;
  if (k >= 3u * per_ch) return;
  const int ch = (int)(k / per_ch); k -= (uint32_t)ch * per_ch;
  const int ty = (int)(k / (uint32_t)P.tiles_x), tx = (int)(k - (uint32_t)ty * (uint32_t)P.tiles_x);
  // the region: grid cells [X0, X0 + R) x [Y0, Y0 + R); of it [lox, hix) x [loy, hiy) (region coordinates) lies inside the grid
  const int R = TILE + 6 * r, X0 = tx * TILE - 3 * r, Y0 = ty * TILE - 3 * r;
  const int lox = max(0, -X0), hix = min(R, P.gw - X0), loy = max(0, -Y0), hiy = min(R, P.gh - Y0);
  const int off = 4 + (X0 & 3);                                    // region column x at byte off + x: a dword where the plane's is
  uint8_t* a = (uint8_t*)buf_a + off; uint8_t* h = (uint8_t*)buf_h + off;
  const size_t plane = (size_t)P.gh * P.gp;
  { // stage: the dwords of the plane's rows that cover [lox, hix); what they hold beyond the grid's last column is never read
    const uint8_t* src = P.cells + ch * plane;
    const int d0 = (X0 + lox) >> 2, d1 = (X0 + hix + 3) >> 2, nd = d1 - d0, ny = hiy - loy;
    for (int i = t; i < ny * nd; i += LEVEL_WG) {
      const int yy = i / nd, d = d0 + (i - yy * nd), y = loy + yy;
      *(uint32_t*)(a + y * PITCH + (4 * d - X0)) = *(const uint32_t*)(src + (size_t)(Y0 + y) * P.gp + 4 * d);
    }
  }
  __syncthreads();
  // D = max, then C = min; each pair of passes gives up the outer r cells of the region
  pass_extrema<true>(a, h, PITCH, 1, loy, hiy, lox, hix, r, t);
  __syncthreads();
  pass_extrema<true>(a, h, 1, PITCH, max(lox, r), min(hix, R - r), loy, hiy, r, t);
  __syncthreads();
  pass_extrema<false>(a, h, PITCH, 1, max(loy, r), min(hiy, R - r), max(lox, r), min(hix, R - r), r, t);
  __syncthreads();
  pass_extrema<false>(a, h, 1, PITCH, max(lox, 2 * r), min(hix, R - 2 * r), max(loy, r), min(hiy, R - r), r, t);
  __syncthreads();
  // the box: rows [ya, yb) summed along x for the tile's columns (a running sum per row), prefix sums down each column, and a
  // tile cell's sum is the difference of two of them
  uint16_t* sx = (uint16_t*)buf_h;                                  // [yb - ya][TILE]
  uint32_t* pre = buf_h + (TILE + 2 * MAX_RADIUS) * TILE / 2;       // [yb - ya][TILE], behind sx
  const int ya = max(loy, 2 * r), yb = min(hiy, R - 2 * r), xa = max(lox, 2 * r), xb = min(hix, R - 2 * r);
  const int tx1 = min(hix, 3 * r + TILE), ty1 = min(hiy, 3 * r + TILE);   // the tile: [3 r, tx1) x [3 r, ty1)
  for (int y = ya + t; y < yb; y += LEVEL_WG) {
    const uint8_t* al = a + y * PITCH;
    int s = 0;
    for (int x = max(xa, 2 * r); x < min(xb, 4 * r); x++) s += al[x];    // the window of column 3 r without its last cell
    for (int x = 3 * r; x < tx1; x++) {
      if (x + r < xb) s += al[x + r];
      if (x - r - 1 >= xa) s -= al[x - r - 1];
      sx[(y - ya) * TILE + (x - 3 * r)] = (uint16_t)s;
    }
  }
  __syncthreads();
  if (t < tx1 - 3 * r) {
    uint32_t run = 0;
    for (int y = ya; y < yb; y++) { run += sx[(y - ya) * TILE + t]; pre[(y - ya) * TILE + t] = run; }
  }
  __syncthreads();
  uint8_t* dst = P.base + ch * plane;
  for (int i = t; i < TILE * TILE; i += LEVEL_WG) {
    const int cy = i / TILE, cx = i - cy * TILE, y = 3 * r + cy, x = 3 * r + cx;
    if (y >= ty1 || x >= tx1) continue;
    const int y0 = max(loy, y - r), y1 = min(hiy - 1, y + r), x0 = max(lox, x - r), x1 = min(hix - 1, x + r);
    const int s = (int)(pre[(y1 - ya) * TILE + cx] - (y0 > ya ? pre[(y0 - 1 - ya) * TILE + cx] : 0u));
    dst[(size_t)(Y0 + y) * P.gp + (X0 + x)] = (uint8_t)box_mean(s, (y1 - y0 + 1) * (x1 - x0 + 1));
  }
}

__global__ __launch_bounds__(WG) void k_flatten_apply(const DevPage* __restrict__ pages, int npages, int floor) {
  __shared__ uint32_t bs[APPLY_CY][APPLY_CX];   // B of the cells around the block: R | G << 8 | B << 16
  const int t = threadIdx.x;
  const DevPage P = pages[find_page(pages, npages, blockIdx.x, BY_BLOCK)];
  const uint32_t k = blockIdx.x - P.block_base;
  if (k >= (uint32_t)P.blocks_y * (uint32_t)P.blocks_x) return;
  const int by = (int)(k / (uint32_t)P.blocks_x), bx = (int)(k - (uint32_t)by * (uint32_t)P.blocks_x);
  const int y0 = by * APPLY_H, x0 = bx * APPLY_W, bh = min(APPLY_H, P.h - y0), bw = min(APPLY_W, P.w - x0);
  const int cy0 = y0 / CELL - 1, cx0 = x0 / CELL - 1;   // axis() of the block's pixels stays inside [c0, c0 + APPLY_C) after clamping
  const size_t plane = (size_t)P.gh * P.gp;
  for (int i = t; i < APPLY_CY * APPLY_CX; i += WG) {
    const int j = i / APPLY_CX, c = i - j * APPLY_CX;
    const size_t at = (size_t)min(max(cy0 + j, 0), P.gh - 1) * P.gp + min(max(cx0 + c, 0), P.gw - 1);
    bs[j][c] = (uint32_t)P.base[at] | ((uint32_t)P.base[plane + at] << 8) | ((uint32_t)P.base[2 * plane + at] << 16);
  }
  __syncthreads();
  const int ipr = items_per_row(bw), items = bh * ipr;
  for (int i = t; i < items; i += WG) {
    const int rrow = i / ipr, j = i - rrow * ipr, y = y0 + rrow;
    const size_t seg = ((size_t)y * P.w + x0) * 3;
    int first;
    const int count = row_item((uintptr_t)(P.dst + seg), bw, j, &first);
    if (count == 0) continue;
    uint32_t px[4];
    load_pixels(P.src + seg + 3 * first, count, px);
    const Axis ay = axis(y, P.gh);
    const uint32_t* r0 = bs[ay.i0 - cy0]; const uint32_t* r1 = bs[ay.i1 - cy0];
    for (int e = 0; e < 4; e++) {
      if (e >= count) break;
      const Axis ax = axis(x0 + first + e, P.gw);
      const uint32_t b00 = r0[ax.i0 - cx0], b01 = r0[ax.i1 - cx0], b10 = r1[ax.i0 - cx0], b11 = r1[ax.i1 - cx0];
      uint32_t o = 0;
      for (int c = 0; c < 3; c++) {
        const int sh = 8 * c;
        const int L = floored(level(ax.w, ay.w, (int)((b00 >> sh) & 255u), (int)((b01 >> sh) & 255u), (int)((b10 >> sh) & 255u),
                                    (int)((b11 >> sh) & 255u)), floor);
        o |= (uint32_t)flat_value_rcp((int)((px[e] >> sh) & 255u), L, __builtin_amdgcn_rcpf((float)L)) << sh;
      }
      px[e] = o;
    }
    store_pixels(P.dst + seg + 3 * first, count, px);
  }
}

}  // namespace

void launch(hipStream_t st, Profiler* prof, const DevPage* d_pages, const DevPage* pages, int n, int radius, int floor) {
  if (n <= 0) return;
  const DevPage& last = pages[n - 1];
  const unsigned strips = last.strip_base + (unsigned)last.gh * (unsigned)last.strips_x;
  const unsigned tiles = last.tile_base + 3u * (unsigned)last.tiles_y * (unsigned)last.tiles_x;
  const unsigned blocks = last.block_base + (unsigned)last.blocks_y * (unsigned)last.blocks_x;
  { ProfScope ps(prof, st, "page_flatten_pool");
    RT_LAUNCH(k_flatten_pool, dim3(strips), dim3(WG), 0, st, d_pages, n); }
  { ProfScope ps(prof, st, "page_flatten_level");
    RT_LAUNCH(k_flatten_level, dim3(tiles), dim3(LEVEL_WG), 0, st, d_pages, n, radius); }
  { ProfScope ps(prof, st, "page_flatten_apply");
    RT_LAUNCH(k_flatten_apply, dim3(blocks), dim3(WG), 0, st, d_pages, n, floor); }
}

}  // namespace pf
}  // namespace rt
