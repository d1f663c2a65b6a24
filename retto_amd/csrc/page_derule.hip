// Page derule on gfx950 (rt_set_page_derule; page_derule.h states the rule): the pages of one lane part in seven launches, without
// global atomics, without synchronisation between workgroups and without a host wait.  The pixels of a page are touched three
// times per pass -- read for the ink bits, read and written by the fill -- and everything in between happens on bit-planes of
// one bit per pixel, 1 / 24 of the page's bytes: a row of 960 pixels is 30 words.
//   k_derule_bits    one workgroup of 256 lanes per strip (4 rows x STRIP_PX pixels) of the part's flat strip list.  The four row
//                    segments go once through LDS as in k_deskew_cells -- cut at the first aligned dword, the body as dwords,
//                    head and tail as bytes, each row at the LDS offset of its own misalignment -- then wave v takes row v: a
//                    lane the luma and the threshold of one pixel, a ballot, and lanes 0 and 1 store the 64 bits: one store
//                    instruction per 64 pixels.  Lanes past w vote 0, so the bits past w are clear.
//   k_derule_hlong   the long horizontal runs: one wave per row, the row's words in registers, word lane * NW + i in register i,
//                    instances NW = 1, 2, 4, 8 by the page's width (2048 pixels per word of a lane).  An opening by a segment
//                    of L pixels: R_1 = B, R_2p[x] = R_p[x] & R_p[x + p] while 2 p <= L, then R_L[x] = R_p[x] & R_p[x + L - p] (the
//                    two windows overlap, which AND does not mind: this is how an L that is no power of two is decomposed); the
//                    dilation back is the mirror image with OR and left shifts.  log2 L + 1 row shifts each.  A row shift by s
//                    bits is one v_alignbit_b32 per word against the next word (the neighbour lane's by ds_bpermute), a
//                    rotation of the lane's registers for the s / 32 mod NW words (compile-time indices: the amounts 1, 2, 4 are
//                    separate instances), and one bpermute per word for the s / 32 / NW lanes; what comes from beyond the row
//                    is 0.  A row whose erosion is empty -- every row of plain text -- skips the dilation.
//   k_derule_vsweep  the long vertical runs: a lane owns one word (32 columns) of one segment of `seg` rows and walks rows; run
//                    lengths are bit-sliced counters, ten planes in registers: increment by ripple carry in word operations,
//                    reset by AND with the row.  The counter starts at 512 - L, so plane 9 IS "length >= L": no comparison, and
//                    a lane stops counting there (saturation).  Erosion (phase 0) walks upwards from seg_end + L - 2 and writes
//                    E[y] = "B[y .. y + L - 1] all set" for the segment's rows; dilation (phase 1) walks downwards from
//                    seg_begin - L + 1 over ~E, counting the rows since the last E, and writes ~plane 9.  The segments are NOT
//                    joined: each lane recomputes the L - 1 rows it needs beyond its segment.  With seg = clamp(L, 32, 128) that
//                    is 2 to 5 times the rows, of planes that are 1 / 24 of the page and stay in L2, and it buys a launch in
//                    which a 960 x 960 page has 30 x 8 .. 30 x 30 independent lanes instead of 30, no second launch for a
//                    join, and no chain between workgroups.
//   k_derule_fill    one workgroup per TILE_H x TILE_W-pixel output tile, an instance per direction.  B and the long-run plane of
//                    the tile and HALO = T_max + 1 bits around it go to LDS (50 rows of 6 words each: 2.4 KB), zero beyond the
//                    page.  No long-run bit in there (the common case): a straight copy, rows cut by the destination address
//                    and moved as whole dwords (page_rows.h).  Otherwise every pixel finds its run's ends, the thin test, the
//                    long test and the fringe from the LDS bits alone -- at most 2 T + 2 bit reads along the pass's thin axis
//                    -- and only a pixel that changes fetches its two sources' pixels (global; they are the few pixels beside
//                    a rule).
// Every loop is bounded by the descriptors; every global address is formed from coordinates inside the page or the planes, every
// LDS bit address from a coordinate within HALO of the tile.
#include "common.h"
#include "page_derule.h"
#include "page_rows.h"
#include "runtime.h"

namespace rt {
namespace pr {
namespace {

using namespace rows;

constexpr int WG = 256;
constexpr int ROW_DW = 3 * (STRIP_PX / 4) + 4;                    // a strip row in LDS: 3072 bytes, up to 3 of misalignment, a spare dword
constexpr int HALO = MAX_THICK + 1, PLANE_W = TILE_W / 32 + 2, PLANE_H = TILE_H + 2 * HALO;
constexpr int PLANES = 10;                                        // 512 - L + L = 512 needs ten bits
static_assert(WG == 64 * STRIP_ROWS && TILE_W % 32 == 0 && HALO <= 32 && MAX_LEN == 1 << (PLANES - 1), "layouts");

enum { BY_STRIP, BY_GROUP, BY_SWEEP, BY_TILE };
// the last page whose base is <= g
__device__ inline int find_page(const DevPage* pages, int n, uint32_t g, int by) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    const DevPage& p = pages[mid];
    const uint32_t b = by == BY_STRIP ? p.strip_base : by == BY_GROUP ? p.group_base : by == BY_SWEEP ? p.sweep_base : p.tile_base;
    if (b <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(WG) void k_derule_bits(const DevPage* __restrict__ pages, int npages, int ink, int pass) {
  __shared__ uint32_t row[STRIP_ROWS][ROW_DW];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const DevPage P = pages[find_page(pages, npages, blockIdx.x, BY_STRIP)];
  const uint32_t k = blockIdx.x - P.strip_base;
  const int groups = (P.h + STRIP_ROWS - 1) / STRIP_ROWS;
  if (k >= (uint32_t)groups * (uint32_t)P.strips_x) return;
  const int gy = (int)(k / (uint32_t)P.strips_x), sx = (int)(k - (uint32_t)gy * (uint32_t)P.strips_x);
  const int x0 = sx * STRIP_PX, y0 = gy * STRIP_ROWS, npx = min(P.w - x0, STRIP_PX), nb = 3 * npx;
  const uint8_t* page = pass ? P.mid : P.src;
  int pad[STRIP_ROWS];
  for (int r = 0; r < STRIP_ROWS; r++) {
    pad[r] = 0;
    if (y0 + r >= P.h) continue;                                    // (a partial group)
    const uint8_t* a = page + ((size_t)(y0 + r) * P.w + x0) * 3;
    pad[r] = (int)((uintptr_t)a & 3);
    const int head = min(nb, (4 - pad[r]) & 3), body = (nb - head) >> 2, tail = nb - head - 4 * body;
    uint8_t* l = (uint8_t*)row[r] + pad[r];                         // segment byte i at l[i]: l + head is a dword where a + head is
    if (t < head) l[t] = a[t];
    if (t < tail) l[head + 4 * body + t] = a[head + 4 * body + t];
    const uint32_t* g = (const uint32_t*)(a + head);
    uint32_t* ld = (uint32_t*)(l + head);
    for (int d = t; d < body; d += WG) ld[d] = g[d];
  }
  __syncthreads();
  const int y = y0 + wave;
  if (y >= P.h) return;
  const uint8_t* l = (const uint8_t*)row[wave] + pad[wave];
  const int w0 = x0 >> 5;
  uint32_t* out = P.bits + (size_t)y * P.wp + w0;
  for (int c = 0; 64 * c < npx; c++) {                               // (uniform in the wave)
    const int x = 64 * c + lane;
    bool v = false;
    if (x < npx) v = is_ink(l[3 * x], l[3 * x + 1], l[3 * x + 2], ink);
    const unsigned long long m = __ballot(v);
    if (lane < 2 && w0 + 2 * c + lane < P.wp) out[2 * c + lane] = lane ? (uint32_t)(m >> 32) : (uint32_t)m;
  }
}

// ---- a row in the registers of a wave: flat word lane * NW + i in w[i] ----------------------------------------------------------
// result word i = source word i + K of the flat row (0 beyond it), 0 < K < NW
template <int NW, int K>
__device__ inline void words_down(uint32_t (&w)[NW], int lane) {
  uint32_t nx[K];
  #pragma unroll
  for (int j = 0; j < K; j++) { nx[j] = (uint32_t)__shfl_down((int)w[j], 1); if (lane == 63) nx[j] = 0u; }
  #pragma unroll
  for (int i = 0; i < NW; i++) w[i] = i + K < NW ? w[i + K < NW ? i + K : 0] : nx[i + K < NW ? 0 : i + K - NW];
}
// result word i = source word i - K (0 before the row), 0 < K < NW
template <int NW, int K>
__device__ inline void words_up(uint32_t (&w)[NW], int lane) {
  uint32_t pv[K];
  #pragma unroll
  for (int j = 0; j < K; j++) { pv[j] = (uint32_t)__shfl_up((int)w[NW - K + j], 1); if (lane == 0) pv[j] = 0u; }
  #pragma unroll
  for (int i = NW - 1; i >= 0; i--) w[i] = i >= K ? w[i >= K ? i - K : 0] : pv[i >= K ? 0 : i];
}
// result bit x = source bit x + s (towards bit 0), zeros from beyond the row; 0 <= s < 32 * 64
template <int NW>
__device__ inline void row_down(uint32_t (&w)[NW], int s, int lane) {
  const int r = s & 31, q = s >> 5, qb = q & (NW - 1), qa = q / NW;   // (s, and so every branch below, is uniform in the wave)
  uint32_t nx = (uint32_t)__shfl_down((int)w[0], 1);
  if (lane == 63) nx = 0u;
  #pragma unroll
  for (int i = 0; i < NW; i++) w[i] = __builtin_amdgcn_alignbit(i + 1 < NW ? w[i + 1 < NW ? i + 1 : 0] : nx, w[i], (uint32_t)r);   // (r = 0: w[i])
  if constexpr (NW > 1) if (qb & 1) words_down<NW, 1>(w, lane);
  if constexpr (NW > 2) if (qb & 2) words_down<NW, 2>(w, lane);
  if constexpr (NW > 4) if (qb & 4) words_down<NW, 4>(w, lane);
  if (qa) {
    #pragma unroll
    for (int i = 0; i < NW; i++) { const uint32_t v = (uint32_t)__shfl_down((int)w[i], (unsigned)qa); w[i] = lane + qa < 64 ? v : 0u; }
  }
}
// result bit x = source bit x - s (away from bit 0), zeros from before the row
template <int NW>
__device__ inline void row_up(uint32_t (&w)[NW], int s, int lane) {
  const int r = s & 31, q = s >> 5, qb = q & (NW - 1), qa = q / NW;
  if (r) {                                                            // (alignbit by 32 - r; r = 0 would give the lower word)
    uint32_t pv = (uint32_t)__shfl_up((int)w[NW - 1], 1);
    if (lane == 0) pv = 0u;
    #pragma unroll
    for (int i = NW - 1; i >= 0; i--) w[i] = __builtin_amdgcn_alignbit(w[i], i > 0 ? w[i > 0 ? i - 1 : 0] : pv, (uint32_t)(32 - r));
  }
  if constexpr (NW > 1) if (qb & 1) words_up<NW, 1>(w, lane);
  if constexpr (NW > 2) if (qb & 2) words_up<NW, 2>(w, lane);
  if constexpr (NW > 4) if (qb & 4) words_up<NW, 4>(w, lane);
  if (qa) {
    #pragma unroll
    for (int i = 0; i < NW; i++) { const uint32_t v = (uint32_t)__shfl_up((int)w[i], (unsigned)qa); w[i] = lane >= qa ? v : 0u; }
  }
}

// the opening of one row of B by a segment of L pixels
template <int NW>
__device__ inline void hlong_row(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int wp, int L, int lane) {
  uint32_t w[NW], s[NW];
  #pragma unroll
  for (int i = 0; i < NW; i++) w[i] = lane * NW + i < wp ? in[lane * NW + i] : 0u;
  int p = 1;
  for (; 2 * p <= L; p *= 2) {
    #pragma unroll
    for (int i = 0; i < NW; i++) s[i] = w[i];
    row_down<NW>(s, p, lane);
    #pragma unroll
    for (int i = 0; i < NW; i++) w[i] &= s[i];
  }
  if (L > p) {
    #pragma unroll
    for (int i = 0; i < NW; i++) s[i] = w[i];
    row_down<NW>(s, L - p, lane);
    #pragma unroll
    for (int i = 0; i < NW; i++) w[i] &= s[i];
  }
  uint32_t any = 0u;
  #pragma unroll
  for (int i = 0; i < NW; i++) any |= w[i];
  if (__ballot(any != 0u) != 0ull) {                                  // (uniform: the wave's row has a run of L)
    for (p = 1; 2 * p <= L; p *= 2) {
      #pragma unroll
      for (int i = 0; i < NW; i++) s[i] = w[i];
      row_up<NW>(s, p, lane);
      #pragma unroll
      for (int i = 0; i < NW; i++) w[i] |= s[i];
    }
    if (L > p) {
      #pragma unroll
      for (int i = 0; i < NW; i++) s[i] = w[i];
      row_up<NW>(s, L - p, lane);
      #pragma unroll
      for (int i = 0; i < NW; i++) w[i] |= s[i];
    }
  }
  #pragma unroll
  for (int i = 0; i < NW; i++)
    if (lane * NW + i < wp) out[lane * NW + i] = w[i];
}

__global__ __launch_bounds__(WG) void k_derule_hlong(const DevPage* __restrict__ pages, int npages, int L) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const DevPage P = pages[find_page(pages, npages, blockIdx.x, BY_GROUP)];
  const uint32_t g = blockIdx.x - P.group_base;
  if (g >= (uint32_t)((P.h + STRIP_ROWS - 1) / STRIP_ROWS)) return;
  const int y = (int)g * STRIP_ROWS + wave;
  if (y >= P.h) return;                                               // (uniform in the wave; no barrier below)
  const uint32_t* in = P.bits + (size_t)y * P.wp;
  uint32_t* out = P.lng + (size_t)y * P.wp;
  if (P.wp <= 64) hlong_row<1>(in, out, P.wp, L, lane);
  else if (P.wp <= 128) hlong_row<2>(in, out, P.wp, L, lane);
  else if (P.wp <= 256) hlong_row<4>(in, out, P.wp, L, lane);
  else hlong_row<8>(in, out, P.wp, L, lane);                          // (wp <= MAX_ROW_WORDS = 512: plan_pages)
}

// phase 0: keep[y] = AND of bits[y .. y + L - 1]; phase 1: lng[y] = OR of keep[y - L + 1 .. y]; rows beyond the page are clear
__global__ __launch_bounds__(SWEEP_WG) void k_derule_vsweep(const DevPage* __restrict__ pages, int npages, int L, int seg, int phase) {
  const DevPage P = pages[find_page(pages, npages, blockIdx.x, BY_SWEEP)];
  const uint64_t g = (uint64_t)(blockIdx.x - P.sweep_base) * SWEEP_WG + threadIdx.x;
  if (g >= (uint64_t)P.nseg * (uint64_t)P.wp) return;
  const int s = (int)(g / (uint32_t)P.wp), wx = (int)(g - (uint64_t)s * (uint32_t)P.wp);
  const int ya = s * seg, yb = ya + min(seg, P.h - ya);               // the rows written: [ya, yb), ya < h as s < nseg
  const int base = MAX_LEN - L;                                       // a counter of value base + n: plane 9 set iff n >= L
  uint32_t bk[PLANES], c[PLANES];
  #pragma unroll
  for (int k = 0; k < PLANES; k++) {
    bk[k] = (base >> k) & 1 ? 0xffffffffu : 0u;
    c[k] = phase == 0 ? bk[k] : (k == PLANES - 1 ? 0xffffffffu : 0u);  // erosion: no run below; dilation: no E above
  }
  const uint32_t* in = (phase == 0 ? P.bits : P.keep) + wx;
  uint32_t* out = (phase == 0 ? P.keep : P.lng) + wx;
  const int first = phase == 0 ? yb + min(L - 1, P.h - yb) - 1 : ya - min(L - 1, ya);
  const int last = phase == 0 ? ya : yb - 1, step = phase == 0 ? -1 : 1;
  const uint32_t flip = phase == 0 ? 0u : 0xffffffffu;
  for (int y = first; y != last + step; y += step) {
    const uint32_t X = in[(size_t)y * P.wp] ^ flip;
    uint32_t carry = X & ~c[PLANES - 1];
    #pragma unroll
    for (int k = 0; k < PLANES; k++) { const uint32_t t = c[k] & carry; c[k] ^= carry; carry = t; }
    #pragma unroll
    for (int k = 0; k < PLANES; k++) c[k] = (c[k] & X) | (bk[k] & ~X);
    if (y >= ya && y < yb) out[(size_t)y * P.wp] = c[PLANES - 1] ^ flip;
  }
}

// DIR 0: the horizontal pass (long runs along x, thin axis y, src -> mid); DIR 1: the vertical pass (mid -> dst)
template <int DIR>
__global__ __launch_bounds__(WG) void k_derule_fill(const DevPage* __restrict__ pages, int npages, int T) {
  __shared__ uint32_t sb[PLANE_H * PLANE_W], sl[PLANE_H * PLANE_W];
  const int t = threadIdx.x;
  const DevPage P = pages[find_page(pages, npages, blockIdx.x, BY_TILE)];
  const uint32_t k = blockIdx.x - P.tile_base;
  if (k >= (uint32_t)P.tiles_y * (uint32_t)P.tiles_x) return;
  const int ty = (int)(k / (uint32_t)P.tiles_x), tx = (int)(k - (uint32_t)ty * (uint32_t)P.tiles_x);
  const int y0 = ty * TILE_H, x0 = tx * TILE_W, bh = min(TILE_H, P.h - y0), bw = min(TILE_W, P.w - x0);
  const uint8_t* in = DIR == 0 ? P.src : P.mid;
  uint8_t* out = DIR == 0 ? P.mid : P.dst;
  const int py = y0 - HALO, pw = (x0 >> 5) - 1;                      // the staged planes' first row and first word
  int any = 0;
  for (int i = t; i < PLANE_H * PLANE_W; i += WG) {
    const int r = i / PLANE_W, y = py + r, wd = pw + i - r * PLANE_W;
    uint32_t b = 0u, l = 0u;
    if (y >= 0 && y < P.h && wd >= 0 && wd < P.wp) { b = P.bits[(size_t)y * P.wp + wd]; l = P.lng[(size_t)y * P.wp + wd]; }
    sb[i] = b; sl[i] = l;
    any |= l != 0u;
  }
  any = __syncthreads_or(any);
  const int ipr = items_per_row(bw), items = bh * ipr;
  for (int i = t; i < items; i += WG) {
    const int rrow = i / ipr, j = i - rrow * ipr, y = y0 + rrow;
    const size_t seg = ((size_t)y * P.w + x0) * 3;
    int first;
    const int count = row_item((uintptr_t)(out + seg), bw, j, &first);
    if (count == 0) continue;
    uint32_t px[4];
    load_pixels(in + seg + 3 * first, count, px);
    for (int e = 0; any && e < count; e++) {                         // (any is uniform: no long run near the tile is a straight copy)
      const int x = x0 + first + e;
      const int u = DIR == 0 ? y : x, n = DIR == 0 ? P.h : P.w;
      // bit (v along the thin axis) of a staged plane: |v - u| <= HALO, so the row is within [0, PLANE_H) and the column within
      // the halo words; beyond the page the planes are 0, which ends every run there
      auto bit = [&](const uint32_t* plane, int v) -> bool {
        const int yy = (DIR == 0 ? v : y) - py, xx = (DIR == 0 ? x : v) - 32 * pw;
        return (plane[yy * PLANE_W + (xx >> 5)] >> (xx & 31)) & 1u;
      };
      auto pixel_at = [&](int v) -> const uint8_t* { return in + ((size_t)(DIR == 0 ? v : y) * P.w + (DIR == 0 ? x : v)) * 3; };
      // the run through the B pixel s (|s - u| <= 1): removable, and then *from = its fill's coordinate
      auto run_fill = [&](int s, int* from) -> bool {
        int u0 = s, u1 = s;
        while (s - u0 < T && bit(sb, u0 - 1)) u0--;
        while (u1 - s < T && bit(sb, u1 + 1)) u1++;
        if (u1 - u0 + 1 > T) return false;
        bool lng = false;
        for (int v = u0; v <= u1; v++) lng = lng || bit(sl, v);
        const bool has_a = u0 >= 2, has_b = u1 + 2 <= n - 1;
        if (!lng || (!has_a && !has_b)) return false;
        const int la = has_a ? luma_of(pixel_at(u0 - 2)) : 0, lb = has_b ? luma_of(pixel_at(u1 + 2)) : 0;
        *from = pick_b(has_a, has_b, la, lb) ? u1 + 2 : u0 - 2;
        return true;
      };
      int from = 0;
      bool hit;
      if (bit(sb, u)) hit = run_fill(u, &from);
      else hit = (bit(sb, u + 1) && run_fill(u + 1, &from)) || (bit(sb, u - 1) && run_fill(u - 1, &from));
      if (hit) { const uint8_t* f = pixel_at(from); px[e] = (uint32_t)f[0] | ((uint32_t)f[1] << 8) | ((uint32_t)f[2] << 16); }
    }
    store_pixels(out + seg + 3 * first, count, px);
  }
}

}  // namespace

void launch(hipStream_t st, Profiler* prof, const DevPage* d_pages, const DevPage* pages, int n, int min_len, int max_thick, int ink) {
  if (n <= 0) return;
  const DevPage& last = pages[n - 1];
  const unsigned groups = (unsigned)((last.h + STRIP_ROWS - 1) / STRIP_ROWS);
  const unsigned n_strips = last.strip_base + groups * (unsigned)last.strips_x, n_groups = last.group_base + groups;
  const unsigned n_sweeps = last.sweep_base + (unsigned)(((uint64_t)last.nseg * last.wp + SWEEP_WG - 1) / SWEEP_WG);
  const unsigned n_tiles = last.tile_base + (unsigned)last.tiles_y * (unsigned)last.tiles_x;
  const int seg = sweep_seg(min_len);
  { ProfScope ps(prof, st, "page_derule_bits");
    RT_LAUNCH(k_derule_bits, dim3(n_strips), dim3(WG), 0, st, d_pages, n, ink, 0); }
  { ProfScope ps(prof, st, "page_derule_hlong");
    RT_LAUNCH(k_derule_hlong, dim3(n_groups), dim3(WG), 0, st, d_pages, n, min_len); }
  { ProfScope ps(prof, st, "page_derule_fill");
    RT_LAUNCH(k_derule_fill<0>, dim3(n_tiles), dim3(WG), 0, st, d_pages, n, max_thick); }
  { ProfScope ps(prof, st, "page_derule_bits");
    RT_LAUNCH(k_derule_bits, dim3(n_strips), dim3(WG), 0, st, d_pages, n, ink, 1); }
  { ProfScope ps(prof, st, "page_derule_vsweep");
    RT_LAUNCH(k_derule_vsweep, dim3(n_sweeps), dim3(SWEEP_WG), 0, st, d_pages, n, min_len, seg, 0); }
  { ProfScope ps(prof, st, "page_derule_vsweep");
    RT_LAUNCH(k_derule_vsweep, dim3(n_sweeps), dim3(SWEEP_WG), 0, st, d_pages, n, min_len, seg, 1); }
  { ProfScope ps(prof, st, "page_derule_fill");
    RT_LAUNCH(k_derule_fill<1>, dim3(n_tiles), dim3(WG), 0, st, d_pages, n, max_thick); }
}

}  // namespace pr
}  // namespace rt
