// Page enhance on gfx950 (rt_set_page_enhance; page_enhance.h states the rule and holds every formula used here): the pages of one
// lane part in two launches, without global atomics and without synchronisation between workgroups.
//   k_enhance_lut    one workgroup of 256 threads (4 waves) per tile of the part's flat tile list: the tile's luma histogram, its
//                    clipping and redistribution, the prefix sum and the 256-byte LUT.
//   k_enhance_apply  one workgroup per cell of the flat cell list (the tile grid shifted by half a tile): the cell's four LUTs in
//                    1 KB of LDS, every pixel looked up four times, blended with its own weights and written to the new page.
// Rows.  A page row is 3 w bytes, so most rows do not start on a dword.  A row segment of n pixels at byte address a is cut into
// items (row_item): the first a & 3 pixels (after k pixels the address is a + 3 k, a dword again at k = a & 3 mod 4), then groups
// of 4 pixels = 12 bytes = three dword accesses, then the rest.  Head and rest are moved as bytes.  k_enhance_apply cuts by its
// destination address; a source of another alignment (a caller's device page at an odd address) is read as bytes.
// The histogram.  A document tile has most of its pixels in one bin -- the paper --, so plain LDS atomics would serialise on one
// address.  Every wave counts into a sub-histogram of its own, and before it touches LDS it aggregates equal values across its
// lanes: the first live lane's value is broadcast, a ballot finds the lanes that hold it, that lane adds the popcount with a plain
// read-modify-write (nobody else writes the wave's sub-histogram meanwhile) and those lanes retire.  A paper tile drains in one
// or two rounds per pixel slot.  After AGG_ROUNDS rounds whatever is still live is scattered enough (noise, a photograph) for one
// atomic each: the rounds are bounded and the worst case stays near the plain form.  Per-lane run counting over the lane's own
// four pixels was the alternative: it divides the number of atomics by at most 4 and still sends 64 lanes to one address.
// Every loop is bounded by the descriptors; every pixel address is formed from coordinates clipped to the page.
#include "common.h"
#include "page_enhance.h"
#include "page_rows.h"
#include "runtime.h"

namespace rt {
namespace pe {
namespace {

constexpr int WG = 256, WAVES = WG / 64, AGG_ROUNDS = 6;

// the last page whose tile_base / cell_base is <= g
__device__ inline int find_page(const DevPage* pages, int n, uint32_t g, bool by_cell) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((by_cell ? pages[mid].cell_base : pages[mid].tile_base) <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}

using namespace rows;   // row_item, load_pixels, store_pixels: page_rows.h
__device__ inline int luma_of(uint32_t px) { return luma((int)(px & 255u), (int)((px >> 8) & 255u), (int)(px >> 16)); }

// One value per lane (live: the lane has one) into the wave's sub-histogram h.  Called by all 64 lanes of the wave together.
__device__ inline void wave_count(uint32_t* h, int v, bool live, int lane) {
  for (int round = 0; round < AGG_ROUNDS; round++) {
    const unsigned long long alive = __ballot(live);
    if (!alive) return;
    const int lead = __ffsll((long long)alive) - 1;
    const int lv = __builtin_amdgcn_readlane(v, lead);
    const bool same = live && v == lv;
    const unsigned long long m = __ballot(same);
    if (lane == lead) { volatile uint32_t* hv = h; hv[lv] = hv[lv] + (uint32_t)__popcll(m); }   // (volatile: another lane's add may lie between two of mine)
    if (same) live = false;
  }
  if (live) atomicAdd(&h[v], 1u);
}

__global__ __launch_bounds__(WG) void k_enhance_lut(const DevPage* __restrict__ pages, int npages, int tile, int clip_x16) {
  __shared__ uint32_t sub[WAVES][256];
  __shared__ uint32_t bins[256];
  __shared__ uint32_t part[WAVES];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const DevPage P = pages[find_page(pages, npages, blockIdx.x, false)];
  const uint32_t k = blockIdx.x - P.tile_base;
  if (k >= (uint32_t)P.nty * (uint32_t)P.ntx) return;
  const int ty = (int)(k / (uint32_t)P.ntx), tx = (int)(k - (uint32_t)ty * (uint32_t)P.ntx);
  const int y0 = ty * tile, y1 = min(P.h, y0 + tile), x0 = tx * tile, x1 = min(P.w, x0 + tile);
  const int tw = x1 - x0, th = y1 - y0, area = tw * th;
  for (int w = 0; w < WAVES; w++) sub[w][t] = 0;
  __syncthreads();
  // the tile's items, 256 at a time: all lanes of a wave run every step, a lane without an item is not live
  const int ipr = items_per_row(tw), items = th * ipr;
  for (int i0 = 0; i0 < items; i0 += WG) {
    const int i = i0 + t;
    int count = 0;
    uint32_t px[4] = {0, 0, 0, 0};
    if (i < items) {
      const int row = i / ipr, j = i - row * ipr;
      const uint8_t* seg = P.src + ((size_t)(y0 + row) * P.w + x0) * 3;
      int first;
      count = row_item((uintptr_t)seg, tw, j, &first);
      load_pixels(seg + 3 * first, count, px);
    }
    for (int e = 0; e < 4; e++) wave_count(sub[wave], luma_of(px[e]), e < count, lane);
  }
  __syncthreads();
  // merge, clip, the excess reduced inside each wave and over the four partial sums, redistribute
  int hc = 0;
  for (int w = 0; w < WAVES; w++) hc += (int)sub[w][t];
  const int L = clip_limit(clip_x16, area);
  int ex = hc > L ? hc - L : 0;
  hc -= ex;
  for (int o = 32; o > 0; o >>= 1) ex += __shfl_xor(ex, o);
  if (lane == 0) part[wave] = (uint32_t)ex;
  __syncthreads();
  int excess = 0;
  for (int w = 0; w < WAVES; w++) excess += (int)part[w];
  bins[t] = (uint32_t)(hc + bin_gain(t, excess));
  __syncthreads();
  // wave 0 scans the 256 bins, four per lane plus a scan across the lanes, and writes the LUT: 64 dwords, coalesced
  if (wave == 0) {
    int c[4], run = 0;
    for (int e = 0; e < 4; e++) { run += (int)bins[4 * lane + e]; c[e] = run; }
    int incl = run;
    for (int o = 1; o < 64; o <<= 1) { const int up = __shfl_up(incl, o); if (lane >= o) incl += up; }
    const int before = incl - run;
    uint32_t word = 0;
    for (int e = 0; e < 4; e++) word |= (uint32_t)lut_value(before + c[e], area) << (8 * e);
    ((uint32_t*)(P.luts + (size_t)k * 256))[lane] = word;
  }
}

__global__ __launch_bounds__(WG) void k_enhance_apply(const DevPage* __restrict__ pages, int npages, int tile) {
  __shared__ uint32_t lut4[256];   // entry Y: a00 | a01 << 8 | a10 << 16 | a11 << 24
  const int t = threadIdx.x;
  const DevPage P = pages[find_page(pages, npages, blockIdx.x, true)];
  const uint32_t k = blockIdx.x - P.cell_base;
  if (k >= (uint32_t)P.ncy * (uint32_t)P.ncx) return;
  const int cy = (int)(k / (uint32_t)P.ncx), cx = (int)(k - (uint32_t)cy * (uint32_t)P.ncx);
  const int y0 = max(0, cy * tile - tile / 2), y1 = min(P.h, cy * tile + tile / 2);
  const int x0 = max(0, cx * tile - tile / 2), x1 = min(P.w, cx * tile + tile / 2);
  if (y0 >= y1 || x0 >= x1) return;
  const Axis ay = axis(y0, tile, P.nty), ax = axis(x0, tile, P.ntx);
  // the four LUTs: 64 lanes fetch 16 bytes each, and spread them into the interleaved table
  if (t < 64) {
    const int q = t >> 4, e0 = (t & 15) * 16;
    const int tyq = q < 2 ? ay.i0 : ay.i1, txq = (q & 1) ? ax.i1 : ax.i0;
    const uint4 v = *(const uint4*)(P.luts + ((size_t)tyq * P.ntx + txq) * 256 + e0);
    const uint32_t words[4] = {v.x, v.y, v.z, v.w};
    uint8_t* tab = (uint8_t*)lut4;
    for (int e = 0; e < 16; e++) tab[(e0 + e) * 4 + q] = (uint8_t)(words[e >> 2] >> (8 * (e & 3)));
  }
  __syncthreads();
  const int cw = x1 - x0, ch = y1 - y0, ipr = items_per_row(cw), items = ch * ipr;
  for (int i = t; i < items; i += WG) {
    const int row = i / ipr, j = i - row * ipr, y = y0 + row;
    const size_t seg = ((size_t)y * P.w + x0) * 3;
    int first;
    const int count = row_item((uintptr_t)(P.dst + seg), cw, j, &first);
    if (count == 0) continue;
    uint32_t px[4];
    load_pixels(P.src + seg + 3 * first, count, px);
    const int wy = cell_weight(ay, y, tile);
    for (int e = 0; e < 4; e++) {
      if (e >= count) break;
      const int r = (int)(px[e] & 255u), g = (int)((px[e] >> 8) & 255u), b = (int)(px[e] >> 16);
      const int Y = luma(r, g, b);
      const uint32_t a = lut4[Y];
      const int wx = cell_weight(ax, x0 + first + e, tile);
      const int d = blend(tile, wx, wy, (int)(a & 255u), (int)((a >> 8) & 255u), (int)((a >> 16) & 255u), (int)(a >> 24)) - Y;
      px[e] = (uint32_t)shift_channel(r, d) | ((uint32_t)shift_channel(g, d) << 8) | ((uint32_t)shift_channel(b, d) << 16);
    }
    store_pixels(P.dst + seg + 3 * first, count, px);
  }
}

}  // namespace

void launch(hipStream_t st, Profiler* prof, const DevPage* d_pages, const DevPage* pages, int n, int tile, int clip_x16) {
  if (n <= 0) return;
  const DevPage& last = pages[n - 1];
  const unsigned tiles = last.tile_base + (unsigned)last.nty * (unsigned)last.ntx;
  const unsigned cells = last.cell_base + (unsigned)last.ncy * (unsigned)last.ncx;
  { ProfScope ps(prof, st, "page_enhance_lut");
    RT_LAUNCH(k_enhance_lut, dim3(tiles), dim3(WG), 0, st, d_pages, n, tile, clip_x16); }
  { ProfScope ps(prof, st, "page_enhance_apply");
    RT_LAUNCH(k_enhance_apply, dim3(cells), dim3(WG), 0, st, d_pages, n, tile); }
}

}  // namespace pe
}  // namespace rt
