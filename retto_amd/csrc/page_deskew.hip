// Page deskew on gfx950 (rt_set_page_deskew; page_deskew.h states the rule and holds every formula used here): the pages of one
// lane part in four launches, without global atomics, without synchronisation between workgroups and without a host wait -- the
// chosen slope stays on the device until the call's results come home.
//   k_deskew_cells    one workgroup of 256 lanes per strip (a row of cells, STRIP_PX pixels of it) of the part's flat strip list.
//                     Four page rows at a time go once through LDS as in k_flatten_pool -- a row segment is cut at its first
//                     aligned dword, the body moves as dwords, head and tail as bytes, each row at the LDS offset of its own
//                     misalignment -- and a lane takes the minimum luma of 4 x 4 pixels from twelve aligned LDS dwords.  Bytes
//                     the strip does not have are 255, whose luma is 255, the identity of min.  A cell of c > 4 pixels is the
//                     minimum over the strip's row groups (a register per lane) and over c / 4 neighbouring lanes (256 bytes of
//                     LDS).  I is written transposed, [gx][gy], the column pitch a whole number of dwords.
//   k_deskew_profile  the hot kernel: one workgroup of 4 waves per page and block of ANGLES_PER_WG = 8 candidate slopes, two per
//                     wave.  For one k the shift d_k is constant along a column, so P_k is a sum of shifted columns.  The grid
//                     is walked in bands of 64 columns (64 x at most 512 bytes = 32 KB), each staged in LDS once with dword
//                     loads and shared by the four waves.  Lane l owns rows l, l + 64, ... of P_k in registers (NR = 4, 6, 8 or
//                     10 per slope, by the page's row count gh + 2 max_shift <= 640); per column it adds I[r - d_k(gx)][gx],
//                     predicated at the ends.  The transposed layout makes a wave's 64 reads 64 consecutive bytes: no bank
//                     conflict, no atomic.  After the last band the wave forms the differences -- lane l's upper neighbour is
//                     lane l + 1's register, lane 63's is lane 0's next register -- squares them in 64 bits, reduces across the
//                     lanes and writes S_k with one store.
//   k_deskew_pick     one wave per page: the argmax of S_k under the tie rule, the gate against S_0, and the page's record
//                     {k*, cosq, sinq} from the angle table.
//   k_deskew_rotate   one workgroup of 256 lanes per 32 x 32-pixel output tile.  k* = 0: a straight copy.  Otherwise the bounding
//                     box of the tile's source footprint is staged in LDS with aligned dword loads (ragged ends as bytes) and the
//                     bilinear blend reads LDS only; output rows are cut by the destination address (page_rows.h) and written as
//                     whole dwords.  The footprint: U is monotone in x and in y, so its extremes over the tile are at corners;
//                     they differ by 2 (cosq (bw - 1) + |sinq| (bh - 1)) <= 2^17 (31 + 31 * 15896 / 65536) < 2^17 * 38.6 (cosq <=
//                     65536, |sinq| <= 15896 at |k*| = 128), so floor(Umax / 2^17) - floor(Umin / 2^17) <= 39, one more column for
//                     the right neighbour: at most 41 columns, and as many rows.  Clamping to the page is monotone and only
//                     shrinks the box.  BOX = 42 rows of 132 bytes: 5.4 KB.
// Every loop is bounded by the descriptors; every address is formed from coordinates clipped to the page, the grid or the box.
#include "common.h"
#include "page_deskew.h"
#include "page_rows.h"
#include "runtime.h"

namespace rt {
namespace pd {
namespace {

using namespace rows;

constexpr int WG = 256, WAVES = WG / 64, ANGLES_PER_WAVE = ANGLES_PER_WG / WAVES, BAND = 64;
constexpr int STRIP_LANE_PX = STRIP_PX / WG;                      // 4 pixels of a row group per lane
constexpr int ROW_DW = 3 * WG + 4;                                // a strip row in LDS: 3072 bytes, up to 3 of misalignment, a spare dword
constexpr int BOX = 42, BOX_PITCH = 132, BOX_PITCH_DW = BOX_PITCH / 4;   // a box row: 3 * 42 bytes and up to 3 of misalignment
static_assert(STRIP_LANE_PX == 4 && ANGLES_PER_WAVE * WAVES == ANGLES_PER_WG && 3 * BOX + 3 <= BOX_PITCH, "layouts");

enum { BY_STRIP, BY_TILE };
// the last page whose strip_base / tile_base is <= g
__device__ inline int find_page(const DevPage* pages, int n, uint32_t g, int by) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    const uint32_t b = by == BY_STRIP ? pages[mid].strip_base : pages[mid].tile_base;
    if (b <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(WG) void k_deskew_cells(const DevPage* __restrict__ pages, int npages) {
  __shared__ uint32_t row[4][ROW_DW];
  __shared__ uint32_t part[WG];
  const int t = threadIdx.x;
  const DevPage P = pages[find_page(pages, npages, blockIdx.x, BY_STRIP)];
  const uint32_t k = blockIdx.x - P.strip_base;
  if (k >= (uint32_t)P.gh * (uint32_t)P.strips_x) return;
  const int gy = (int)(k / (uint32_t)P.strips_x), sx = (int)(k - (uint32_t)gy * (uint32_t)P.strips_x);
  const int cell0 = sx * P.cells_per_strip;
  uint32_t m = 255u;
  for (int piece = 0; piece < P.pieces; piece++) {
    const long long xs = (long long)cell0 * P.c + (long long)piece * STRIP_PX;
    if (xs >= P.w) break;
    const int x0 = (int)xs, npx = min(P.w - x0, STRIP_PX), nb = 3 * npx;
    for (int yg = 0; yg < P.c; yg += 4) {
      const long long ys = (long long)gy * P.c + yg;
      if (ys >= P.h) break;
      const int y0 = (int)ys;
      __syncthreads();                                              // (the previous group has been read)
      for (int i = t; i < 4 * ROW_DW; i += WG) (&row[0][0])[i] = 0xffffffffu;
      __syncthreads();
      int pad[4];
      for (int r = 0; r < 4; r++) {
        pad[r] = 0;
        if (y0 + r >= P.h) continue;                                // (a partial group: the missing rows stay 255)
        const uint8_t* a = P.src + ((size_t)(y0 + r) * P.w + x0) * 3;
        pad[r] = (int)((uintptr_t)a & 3);
        const int head = min(nb, (4 - pad[r]) & 3), body = (nb - head) >> 2, tail = nb - head - 4 * body;
        uint8_t* l = (uint8_t*)row[r] + pad[r];                     // segment byte i at l[i]: l + head is a dword where a + head is
        if (t < head) l[t] = a[t];
        if (t < tail) l[head + 4 * body + t] = a[head + 4 * body + t];
        const uint32_t* g = (const uint32_t*)(a + head);
        uint32_t* ld = (uint32_t*)(l + head);
        for (int d = t; d < body; d += WG) ld[d] = g[d];
      }
      __syncthreads();
      for (int r = 0; r < 4; r++) {
        const uint32_t* q = &row[r][3 * t];
        const uint32_t q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
        const int sh = 8 * pad[r];
        const uint32_t w0 = (uint32_t)((((uint64_t)q1 << 32) | q0) >> sh), w1 = (uint32_t)((((uint64_t)q2 << 32) | q1) >> sh),
                       w2 = (uint32_t)((((uint64_t)q3 << 32) | q2) >> sh);   // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
        const uint32_t l0 = (uint32_t)pe::luma((int)(w0 & 255u), (int)((w0 >> 8) & 255u), (int)((w0 >> 16) & 255u));
        const uint32_t l1 = (uint32_t)pe::luma((int)(w0 >> 24), (int)(w1 & 255u), (int)((w1 >> 8) & 255u));
        const uint32_t l2 = (uint32_t)pe::luma((int)((w1 >> 16) & 255u), (int)(w1 >> 24), (int)(w2 & 255u));
        const uint32_t l3 = (uint32_t)pe::luma((int)((w2 >> 8) & 255u), (int)((w2 >> 16) & 255u), (int)(w2 >> 24));
        m = min(m, min(min(l0, l1), min(l2, l3)));
      }
    }
  }
  part[t] = m;
  __syncthreads();
  // lanes to cells: a cell is c / 4 neighbouring lanes, or the whole workgroup where it is STRIP_PX pixels or wider
  const int lanes_per_cell = min(P.c / STRIP_LANE_PX, WG);
  if (t >= P.cells_per_strip || cell0 + t >= P.gw) return;
  uint32_t v = 255u;
  for (int i = 0; i < lanes_per_cell; i++) v = min(v, part[t * lanes_per_cell + i]);
  P.cells[(size_t)(cell0 + t) * P.gp + gy] = (uint8_t)(255u - v);
}

__device__ inline uint64_t wave_sum(uint64_t s) {
  uint32_t lo = (uint32_t)s, hi = (uint32_t)(s >> 32);
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t o = ((uint64_t)(uint32_t)__shfl_xor((int)hi, off) << 32) | (uint32_t)__shfl_xor((int)lo, off);
    s += o; lo = (uint32_t)s; hi = (uint32_t)(s >> 32);
  }
  return s;
}

// the profiles of one page for the workgroup's slopes: NR row registers per slope and lane
template <int NR>
__device__ inline void profile_rows(const DevPage& P, int K, int blk, uint32_t* band) {
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int D = max_shift(P.gw, K);
  uint32_t acc[ANGLES_PER_WAVE][NR];
  int idx[ANGLES_PER_WAVE];
  for (int a = 0; a < ANGLES_PER_WAVE; a++) {
    idx[a] = blk * ANGLES_PER_WG + wave * ANGLES_PER_WAVE + a;       // slope idx - K; beyond 2 K: none
    for (int j = 0; j < NR; j++) acc[a][j] = 0u;
  }
  const uint8_t* bytes = (const uint8_t*)band;
  for (int c0 = 0; c0 < P.gw; c0 += BAND) {
    const int nc = min(BAND, P.gw - c0), ndw = nc * (P.gp >> 2);
    __syncthreads();                                                 // (the previous band has been read)
    const uint32_t* src = (const uint32_t*)(P.cells + (size_t)c0 * P.gp);
    for (int i = t; i < ndw; i += WG) band[i] = src[i];
    __syncthreads();
    #pragma unroll
    for (int a = 0; a < ANGLES_PER_WAVE; a++) {
      if (idx[a] > 2 * K) continue;
      const int k = idx[a] - K;
      for (int col = 0; col < nc; col++) {
        const int base = lane - D - shift_of(c0 + col, P.gw, k);     // row R = gy + d + D of P_k, so gy = R - D - d
        const uint8_t* cp = bytes + col * P.gp;
        #pragma unroll
        for (int j = 0; j < NR; j++) {
          const int gy = base + 64 * j;
          if ((unsigned)gy < (unsigned)P.gh) acc[a][j] += cp[gy];
        }
      }
    }
  }
  #pragma unroll
  for (int a = 0; a < ANGLES_PER_WAVE; a++) {
    if (idx[a] > 2 * K) continue;                                    // (uniform in the wave)
    uint32_t rot[NR + 1];
    #pragma unroll
    for (int j = 0; j < NR; j++) rot[j] = (uint32_t)__shfl((int)acc[a][j], (lane + 1) & 63);
    rot[NR] = 0u;                                                    // the zero row above the last
    uint64_t s = lane == 0 ? (uint64_t)acc[a][0] * acc[a][0] : 0ull; // the zero row below the first
    #pragma unroll
    for (int j = 0; j < NR; j++) {
      const long long df = (long long)(lane == 63 ? rot[j + 1] : rot[j]) - (long long)acc[a][j];
      s += (uint64_t)(df * df);
    }
    s = wave_sum(s);
    if (lane == 0) P.scores[idx[a]] = s;
  }
}

__global__ __launch_bounds__(WG) void k_deskew_profile(const DevPage* __restrict__ pages, int K, int ablocks) {
  __shared__ uint32_t band[BAND * MAX_GRID / 4];
  const int page = (int)(blockIdx.x / (uint32_t)ablocks), blk = (int)(blockIdx.x - (uint32_t)page * (uint32_t)ablocks);
  const DevPage P = pages[page];
  const int nr = (P.gh + 2 * max_shift(P.gw, K) + 63) >> 6;          // <= 10: gh <= 512, max_shift <= 64
  if (nr <= 4) profile_rows<4>(P, K, blk, band);
  else if (nr <= 6) profile_rows<6>(P, K, blk, band);
  else if (nr <= 8) profile_rows<8>(P, K, blk, band);
  else profile_rows<10>(P, K, blk, band);
}

__global__ __launch_bounds__(64) void k_deskew_pick(const DevPage* __restrict__ pages, int K, int min_gain, const int32_t* __restrict__ table) {
  const DevPage P = pages[blockIdx.x];
  const int lane = threadIdx.x;
  const uint64_t s0 = P.scores[K];
  uint64_t bs = s0; int bk = 0;
  for (int i = lane; i <= 2 * K; i += 64) {
    const uint64_t s = P.scores[i];
    if (better(s, i - K, bs, bk)) { bs = s; bk = i - K; }
  }
  for (int off = 32; off > 0; off >>= 1) {                           // (a strict total order: every lane ends with the same pair)
    const uint64_t os = ((uint64_t)(uint32_t)__shfl_xor((int)(bs >> 32), off) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)bs, off);
    const int ok = __shfl_xor(bk, off);
    if (better(os, ok, bs, bk)) { bs = os; bk = ok; }
  }
  if (lane != 0) return;
  if (gated(bs, s0, min_gain)) bk = 0;
  const int a = bk < 0 ? -bk : bk;
  *P.rec = Record{bk, table[2 * a], bk < 0 ? -table[2 * a + 1] : table[2 * a + 1]};
}

__global__ __launch_bounds__(WG) void k_deskew_rotate(const DevPage* __restrict__ pages, int npages) {
  __shared__ uint32_t box[BOX * BOX_PITCH_DW];
  const int t = threadIdx.x;
  const DevPage P = pages[find_page(pages, npages, blockIdx.x, BY_TILE)];
  const uint32_t k = blockIdx.x - P.tile_base;
  if (k >= (uint32_t)P.tiles_y * (uint32_t)P.tiles_x) return;
  const int ty = (int)(k / (uint32_t)P.tiles_x), tx = (int)(k - (uint32_t)ty * (uint32_t)P.tiles_x);
  const int y0 = ty * TILE, x0 = tx * TILE, bh = min(TILE, P.h - y0), bw = min(TILE, P.w - x0);
  const Record rec = *P.rec;
  const int ipr = items_per_row(bw), items = bh * ipr;
  if (rec.k == 0) {                                                  // (uniform in the workgroup)
    for (int i = t; i < items; i += WG) {
      const int rrow = i / ipr, j = i - rrow * ipr;
      const size_t seg = ((size_t)(y0 + rrow) * P.w + x0) * 3;
      int first;
      const int count = row_item((uintptr_t)(P.dst + seg), bw, j, &first);
      if (count == 0) continue;
      uint32_t px[4];
      load_pixels(P.src + seg + 3 * first, count, px);
      store_pixels(P.dst + seg + 3 * first, count, px);
    }
    return;
  }
  // the box: U and V are monotone along x and along y, so the tile's corners bound them
  const int xe = x0 + bw - 1, ye = y0 + bh - 1;
  const long long ua = turn_u(x0, y0, P.h, P.w, rec.cosq, rec.sinq), ub = turn_u(xe, y0, P.h, P.w, rec.cosq, rec.sinq),
                  uc = turn_u(x0, ye, P.h, P.w, rec.cosq, rec.sinq), ud = turn_u(xe, ye, P.h, P.w, rec.cosq, rec.sinq);
  const long long va = turn_v(x0, y0, P.h, P.w, rec.cosq, rec.sinq), vb = turn_v(xe, y0, P.h, P.w, rec.cosq, rec.sinq),
                  vc = turn_v(x0, ye, P.h, P.w, rec.cosq, rec.sinq), vd = turn_v(xe, ye, P.h, P.w, rec.cosq, rec.sinq);
  const int bx0 = clampi(min(min(ua, ub), min(uc, ud)) >> 17, P.w - 1), bx1 = clampi((max(max(ua, ub), max(uc, ud)) >> 17) + 1, P.w - 1);
  const int by0 = clampi(min(min(va, vb), min(vc, vd)) >> 17, P.h - 1), by1 = clampi((max(max(va, vb), max(vc, vd)) >> 17) + 1, P.h - 1);
  const int nbx = min(bx1 - bx0 + 1, BOX), nby = min(by1 - by0 + 1, BOX), nb = 3 * nbx;   // (<= 41 each way: the bound above)
  const uintptr_t a0 = (uintptr_t)P.src + ((size_t)by0 * P.w + bx0) * 3;
  const int row_step = (int)((3u * (uint32_t)P.w) & 3u);             // a box row's misalignment: (a0 + r * 3 w) & 3
  // stage: LDS dword d of box row r holds the bytes [4 d - pad, 4 d - pad + 4) of the row's segment; whole dwords are aligned loads
  for (int i = t; i < nby * BOX_PITCH_DW; i += WG) {
    const int r = i / BOX_PITCH_DW, d = i - r * BOX_PITCH_DW;
    const uint8_t* a = P.src + ((size_t)(by0 + r) * P.w + bx0) * 3;
    const int lo = 4 * d - (int)((uintptr_t)a & 3);
    uint32_t v = 0u;
    if (lo >= 0 && lo + 4 <= nb) v = *(const uint32_t*)(a + lo);
    else
      for (int b = 0; b < 4; b++)
        if (lo + b >= 0 && lo + b < nb) v |= (uint32_t)a[lo + b] << (8 * b);
    box[i] = v;
  }
  __syncthreads();
  const uint8_t* bb = (const uint8_t*)box;
  for (int i = t; i < items; i += WG) {
    const int rrow = i / ipr, j = i - rrow * ipr, y = y0 + rrow;
    const size_t seg = ((size_t)y * P.w + x0) * 3;
    int first;
    const int count = row_item((uintptr_t)(P.dst + seg), bw, j, &first);
    if (count == 0) continue;
    uint32_t px[4] = {0u, 0u, 0u, 0u};
    for (int e = 0; e < 4; e++) {
      if (e >= count) break;
      const Sample s = sample_at(x0 + first + e, y, P.h, P.w, rec.cosq, rec.sinq);
      // (inside the box by the bound above; the clips only keep the LDS index in range whatever happens)
      const int r0 = min(max(s.y0 - by0, 0), nby - 1), r1 = min(max(s.y1 - by0, 0), nby - 1);
      const int c0 = 3 * min(max(s.x0 - bx0, 0), nbx - 1), c1 = 3 * min(max(s.x1 - bx0, 0), nbx - 1);
      const uint8_t* q0 = bb + r0 * BOX_PITCH + (int)((a0 + (uintptr_t)(r0 * row_step)) & 3);
      const uint8_t* q1 = bb + r1 * BOX_PITCH + (int)((a0 + (uintptr_t)(r1 * row_step)) & 3);
      uint32_t o = 0u;
      for (int ch = 0; ch < 3; ch++) o |= (uint32_t)blend(s.fu, s.fv, q0[c0 + ch], q0[c1 + ch], q1[c0 + ch], q1[c1 + ch]) << (8 * ch);
      px[e] = o;
    }
    store_pixels(P.dst + seg + 3 * first, count, px);
  }
}

}  // namespace

void launch(hipStream_t st, Profiler* prof, const DevPage* d_pages, const DevPage* pages, int n, int K, int min_gain, const int32_t* d_table) {
  if (n <= 0) return;
  const DevPage& last = pages[n - 1];
  const unsigned strips = last.strip_base + (unsigned)last.gh * (unsigned)last.strips_x;
  const unsigned tiles = last.tile_base + (unsigned)last.tiles_y * (unsigned)last.tiles_x;
  const int ablocks = angle_blocks(K);
  { ProfScope ps(prof, st, "page_deskew_cells");
    RT_LAUNCH(k_deskew_cells, dim3(strips), dim3(WG), 0, st, d_pages, n); }
  { ProfScope ps(prof, st, "page_deskew_profile");
    RT_LAUNCH(k_deskew_profile, dim3((unsigned)n * (unsigned)ablocks), dim3(WG), 0, st, d_pages, K, ablocks); }
  { ProfScope ps(prof, st, "page_deskew_pick");
    RT_LAUNCH(k_deskew_pick, dim3((unsigned)n), dim3(64), 0, st, d_pages, K, min_gain, d_table); }
  { ProfScope ps(prof, st, "page_deskew_rotate");
    RT_LAUNCH(k_deskew_rotate, dim3(tiles), dim3(WG), 0, st, d_pages, n); }
}

}  // namespace pd
}  // namespace rt
