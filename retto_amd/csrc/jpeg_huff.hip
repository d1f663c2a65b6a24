// JPEG entropy decoding on gfx950 for the pages of one lane part (rt_set_jpeg_entropy mode 1): baseline Huffman scans straight
// into the int16 coefficient planes k_jpeg_idct reads.  Self-synchronising parallel Huffman decoding, one lane per subsequence of
// HUFF_S bits of the unstuffed stream (jpeg_huff.h has the method, the lane state and the shared decode step):
//   k_huff_zero   clears the coefficient planes (the write pass stores non-zero coefficients only)
//   k_huff_sync   pass 1: every lane decodes its subsequence from a guessed state, then on into the following ones of its
//                 workgroup, replacing the stored exit states until its own agrees.  The workgroup's window of the stream and the
//                 page's six Huffman tables are staged in LDS first, so the lanes' byte reads and table lookups are LDS reads;
//                 the exit states live in LDS for the rounds.
//   k_huff_link   pass 2: the same overflow step across workgroup boundaries, one lane per boundary, one workgroup per page
//   k_huff_scan   pass 3: per segment, prefix sum of the completed-block counts -> every subsequence's first block
//   k_huff_write  pass 4: every lane decodes its subsequence once more from its now-true entry state into the planes (DC as its
//                 difference), and checks that its exit state is the stored one -- an unbroken chain of such checks from a
//                 segment's first bit is the serial decode -- and at a segment's end the predicted block count
//   k_huff_dc     pass 5: per segment and component, prefix sum of the DC differences in scan order (wrap-around uint32, as the
//                 host's predictor), int16 range check
// A page any lane cannot prove equal to the host's reading gets its flag set; the caller decodes it on the host.  Every loop is
// bounded: a decode step consumes a bit, the rounds are capped at their worst case and the cap sets the flag.
#include "common.h"
#include "jpeg_huff.h"

namespace rt {
namespace {

using namespace jpeg;

// the last page whose wg_base / seg_base is <= v (both strictly increase: every page has a workgroup and a segment)
__device__ inline int find_page(const DevHuffPage* pages, int npages, uint32_t v, bool by_seg) {
  int lo = 0, hi = npages - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((by_seg ? pages[mid].seg_base : pages[mid].wg_base) <= v) lo = mid; else hi = mid - 1;
  }
  return lo;
}
__device__ inline HuffSeg find_seg(const HuffSeg* segs, uint32_t nsegs, uint32_t sub) {
  uint32_t lo = 0, hi = nsegs - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (segs[mid].first_sub <= sub) lo = mid; else hi = mid - 1;
  }
  return segs[lo];
}
__device__ inline bool same_state(const HuffState& a, const HuffState& b) { return a.p == b.p && a.kz == b.kz && a.n == b.n; }

// inclusive prefix sum over the workgroup's 256 lanes; sc[255] is the total until the caller's next barrier
__device__ inline uint32_t block_scan(uint32_t v, uint32_t* sc) {
  const int t = threadIdx.x;
  sc[t] = v;
  __syncthreads();
  for (int off = 1; off < HUFF_WG; off <<= 1) {
    const uint32_t a = t >= off ? sc[t - off] : 0;
    __syncthreads();
    sc[t] += a;
    __syncthreads();
  }
  return sc[t];
}

struct Window {
  HuffTab tabs[6];
  alignas(16) uint8_t bytes[HUFF_WG * HUFF_SUB_BYTES + HUFF_PAD];
};
// the page's tables and the stream bytes of subsequences [sub0, sub0 + here) plus the pad, as 32-bit words
__device__ inline void stage(Window& w, const uint8_t* base, const DevHuffPage& P, uint32_t sub0, uint32_t here) {
  const uint32_t* t = (const uint32_t*)(base + P.tabs_off);
  for (uint32_t i = threadIdx.x; i < 6 * sizeof(HuffTab) / 4; i += HUFF_WG) ((uint32_t*)w.tabs)[i] = t[i];
  const uint32_t* s = (const uint32_t*)(base + P.stream_off + (size_t)sub0 * HUFF_SUB_BYTES);
  for (uint32_t i = threadIdx.x; i < (here * HUFF_SUB_BYTES + HUFF_PAD) / 4; i += HUFF_WG) ((uint32_t*)w.bytes)[i] = s[i];
  __syncthreads();
}

__global__ __launch_bounds__(256) void k_huff_zero(uint8_t* __restrict__ base, const DevHuffPage* __restrict__ pages) {
  const DevHuffPage& P = pages[blockIdx.y / 3];
  const int c = blockIdx.y % 3;
  if (c >= P.G.nc) return;
  uint4* p = (uint4*)(base + P.coef_off[c]);
  const uint32_t n = P.coef_bytes[c] / 16;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = make_uint4(0, 0, 0, 0);
}

__global__ __launch_bounds__(HUFF_WG) void k_huff_sync(uint8_t* __restrict__ base, const DevHuffPage* __restrict__ pages, int npages,
                                                       int* __restrict__ info) {
  __shared__ Window w;
  __shared__ HuffState exits[HUFF_WG];
  const int pi = find_page(pages, npages, blockIdx.x, false);
  const DevHuffPage& P = pages[pi];
  const uint32_t sub0 = (blockIdx.x - P.wg_base) * HUFF_WG;
  const uint32_t here = P.nsubs - sub0 < (uint32_t)HUFF_WG ? P.nsubs - sub0 : (uint32_t)HUFF_WG;
  stage(w, base, P, sub0, here);
  const uint32_t i = threadIdx.x, limit = here * HUFF_SUB_BYTES + HUFF_PAD;
  bool act = i < here;
  HuffSeg sg{};
  uint32_t cur = 0, nss = 0;   // the subsequence (within its segment) this lane decodes next; the segment's subsequences
  int seg_byte = 0;            // the segment's first byte relative to the window (negative: it began in an earlier workgroup)
  HuffState st{0, 0, 0};
  if (act) {
    sg = find_seg((const HuffSeg*)(base + P.segs_off), P.nsegs, sub0 + i);
    cur = sub0 + i - sg.first_sub;
    nss = huff_seg_subs(sg);
    seg_byte = ((int)sg.first_sub - (int)sub0) * HUFF_SUB_BYTES;
    st.p = cur * HUFF_S;   // the guess: a block starts at my first bit (true for a segment's first subsequence)
  }
  HuffNoSink sink;
  int rounds = 0;
  for (;;) {
    if (!__syncthreads_or(act)) break;
    if (rounds == HUFF_WG) { if (i == 0) atomicOr(&info[pi * HUFF_INFO], 1); break; }
    if (act) {   // round r: lane i is at subsequence i + r, alone; the slot holds what lanes above i left in earlier rounds
      const uint32_t end = (cur + 1) * HUFF_S < sg.nbits ? (cur + 1) * HUFF_S : sg.nbits;
      const int status = huff_decode_sub(w.tabs, P.G, w.bytes, seg_byte, limit, sg.nbits, end, st, sink);
      const uint32_t li = sg.first_sub + cur - sub0;
      if (status == HUFF_BAD) {   // a wrong guess ends here; the lane that owns the truth overwrites (pass 4 flags a true BAD)
        if (rounds == 0) exits[li] = HuffState{HUFF_INVALID, 0, 0};
        act = false;
      } else if (rounds > 0 && same_state(exits[li], st)) {
        act = false;
      } else {
        exits[li] = st;
        cur++;
        if (cur >= nss || li + 1 >= here) act = false;
      }
    }
    rounds++;
  }
  HuffState* states = (HuffState*)(base + P.state_off);
  if (i < here) states[sub0 + i] = exits[i];
  if (i == 0) atomicMax(&info[pi * HUFF_INFO + 1], rounds);
}

// lane b: the boundary behind workgroup b of pass 1.  A round takes it through one workgroup's range, so in a round the lanes work
// on disjoint ranges and a lane always comes after the lanes above it -- the order pass 1's rounds have.
__global__ __launch_bounds__(HUFF_MAX_WGS) void k_huff_link(uint8_t* __restrict__ base, const DevHuffPage* __restrict__ pages,
                                                            int* __restrict__ info) {
  const DevHuffPage& P = pages[blockIdx.x];
  if (P.nwg < 2) return;
  const HuffTab* tabs = (const HuffTab*)(base + P.tabs_off);
  HuffState* states = (HuffState*)(base + P.state_off);
  const uint8_t* s = base + P.stream_off;
  const uint32_t b = threadIdx.x, limit = P.nsubs * HUFF_SUB_BYTES + HUFF_PAD;
  bool act = b + 1 < P.nwg;
  HuffSeg sg{};
  uint32_t cur = 0, nss = 0;
  HuffState st{0, 0, 0};
  if (act) {
    const uint32_t j = (b + 1) * HUFF_WG;
    sg = find_seg((const HuffSeg*)(base + P.segs_off), P.nsegs, j);
    st = states[j - 1];
    cur = j - sg.first_sub; nss = huff_seg_subs(sg);
    if (cur == 0 || st.p == HUFF_INVALID) act = false;   // a segment starts here (true by construction) / nothing to carry over
  }
  HuffNoSink sink;
  int rounds = 0;
  for (;;) {
    if (!__syncthreads_or(act)) break;
    if (rounds == (int)P.nwg) { if (b == 0) atomicOr(&info[blockIdx.x * HUFF_INFO], 1); break; }
    for (int step = 0; step < HUFF_WG && act; step++) {
      const uint32_t end = (cur + 1) * HUFF_S < sg.nbits ? (cur + 1) * HUFF_S : sg.nbits;
      const int status = huff_decode_sub(tabs, P.G, s, (int)(sg.first_sub * HUFF_SUB_BYTES), limit, sg.nbits, end, st, sink);
      HuffState* slot = states + sg.first_sub + cur;
      if (status == HUFF_BAD || same_state(*slot, st)) { act = false; break; }
      *slot = st;
      cur++;
      if (cur >= nss) act = false;
    }
    __threadfence_block();
    rounds++;
  }
  if (b == 0) atomicMax(&info[blockIdx.x * HUFF_INFO + 2], rounds);
}

__global__ __launch_bounds__(HUFF_WG) void k_huff_scan(uint8_t* __restrict__ base, const DevHuffPage* __restrict__ pages, int npages) {
  __shared__ uint32_t sc[HUFF_WG];
  const DevHuffPage& P = pages[find_page(pages, npages, blockIdx.x, true)];
  const HuffSeg sg = ((const HuffSeg*)(base + P.segs_off))[blockIdx.x - P.seg_base];
  const HuffState* states = (const HuffState*)(base + P.state_off) + sg.first_sub;
  uint32_t* first = (uint32_t*)(base + P.first_off) + sg.first_sub;
  const uint32_t nss = huff_seg_subs(sg);
  uint32_t carry = sg.first_mcu * (uint32_t)P.G.bpm;
  for (uint32_t i0 = 0; i0 < nss; i0 += HUFF_WG) {
    const uint32_t i = i0 + threadIdx.x;
    const uint32_t v = i < nss ? states[i].n : 0;
    const uint32_t incl = block_scan(v, sc);
    if (i < nss) first[i] = carry + incl - v;
    carry += sc[HUFF_WG - 1];
    __syncthreads();
  }
}

__global__ __launch_bounds__(HUFF_WG) void k_huff_write(uint8_t* __restrict__ base, const DevHuffPage* __restrict__ pages, int npages,
                                                        int* __restrict__ info) {
  __shared__ Window w;
  const int pi = find_page(pages, npages, blockIdx.x, false);
  const DevHuffPage& P = pages[pi];
  const uint32_t sub0 = (blockIdx.x - P.wg_base) * HUFF_WG;
  const uint32_t here = P.nsubs - sub0 < (uint32_t)HUFF_WG ? P.nsubs - sub0 : (uint32_t)HUFF_WG;
  stage(w, base, P, sub0, here);
  const uint32_t i = threadIdx.x, j = sub0 + i;
  if (i >= here) return;
  const HuffSeg sg = find_seg((const HuffSeg*)(base + P.segs_off), P.nsegs, j);
  const HuffState* states = (const HuffState*)(base + P.state_off);
  const uint32_t cur = j - sg.first_sub, nss = huff_seg_subs(sg);
  HuffState st{0, 0, 0};
  if (cur > 0) {
    st = states[j - 1];
    if (st.p == HUFF_INVALID) { atomicOr(&info[pi * HUFF_INFO], 1); return; }
  }
  HuffCoefSink sink;
  sink.G = &P.G;
  for (int c = 0; c < 3; c++) sink.plane[c] = (int16_t*)(base + P.coef_off[c]);
  sink.first = ((const uint32_t*)(base + P.first_off))[j];
  sink.seg_end = (sg.first_mcu + sg.n_mcus) * (uint32_t)P.G.bpm;
  const uint32_t end = (cur + 1) * HUFF_S < sg.nbits ? (cur + 1) * HUFF_S : sg.nbits;
  const int status = huff_decode_sub(w.tabs, P.G, w.bytes, ((int)sg.first_sub - (int)sub0) * HUFF_SUB_BYTES,
                                     here * HUFF_SUB_BYTES + HUFF_PAD, sg.nbits, end, st, sink);
  if (status == HUFF_BAD || !same_state(states[j], st) || (cur == nss - 1 && !huff_seg_end_ok(sg, P.G, st, sink.first)))
    atomicOr(&info[pi * HUFF_INFO], 1);
}

constexpr int DC_PER_LANE = 8;
__global__ __launch_bounds__(HUFF_WG) void k_huff_dc(uint8_t* __restrict__ base, const DevHuffPage* __restrict__ pages, int npages,
                                                     int* __restrict__ info) {
  __shared__ uint32_t sc[HUFF_WG];
  const uint32_t si = blockIdx.x / 3;
  const int c = blockIdx.x % 3;
  const int pi = find_page(pages, npages, si, true);
  const DevHuffPage& P = pages[pi];
  if (c >= P.G.nc) return;
  const HuffSeg sg = ((const HuffSeg*)(base + P.segs_off))[si - P.seg_base];
  int16_t* plane = (int16_t*)(base + P.coef_off[c]);
  const uint32_t n = sg.n_mcus * (uint32_t)(P.G.hs[c] * P.G.vs[c]);
  uint32_t carry = 0;
  bool wide = false;
  for (uint32_t i0 = 0; i0 < n; i0 += HUFF_WG * DC_PER_LANE) {
    const uint32_t mine = i0 + threadIdx.x * DC_PER_LANE;
    uint32_t at[DC_PER_LANE], run[DC_PER_LANE], sum = 0;
    for (int e = 0; e < DC_PER_LANE; e++) {
      at[e] = mine + e < n ? (uint32_t)huff_comp_block_pos(P.G, c, sg.first_mcu, mine + e) : 0;
      if (mine + e < n) sum += (uint32_t)(int)plane[at[e]];
      run[e] = sum;
    }
    const uint32_t before = carry + block_scan(sum, sc) - sum;
    for (int e = 0; e < DC_PER_LANE; e++) {
      if (mine + e >= n) break;
      const int pred = (int)(before + run[e]);   // (unsigned)pred + (unsigned)diff, as JpegDec::decode_block
      wide |= pred < -32768 || pred > 32767;
      plane[at[e]] = (int16_t)pred;
    }
    carry += sc[HUFF_WG - 1];
    __syncthreads();
  }
  if (wide) atomicOr(&info[pi * HUFF_INFO], 1);
}

}  // namespace

void launch_jpeg_huff(uint8_t* base, const jpeg::DevHuffPage* pages, int* info, const jpeg::DevHuffPage* hpages, int npages,
                      hipStream_t st) {
  if (npages <= 0) return;
  const jpeg::DevHuffPage& L = hpages[npages - 1];
  const unsigned wgs = L.wg_base + L.nwg, segs = L.seg_base + L.nsegs;
  bool link = false;
  for (int i = 0; i < npages; i++) link |= hpages[i].nwg > 1;
  RT_LAUNCH(k_huff_zero, dim3(64, (unsigned)npages * 3), dim3(256), 0, st, base, pages);
  RT_LAUNCH(k_huff_sync, dim3(wgs), dim3(jpeg::HUFF_WG), 0, st, base, pages, npages, info);
  if (link) RT_LAUNCH(k_huff_link, dim3((unsigned)npages), dim3(jpeg::HUFF_MAX_WGS), 0, st, base, pages, info);
  RT_LAUNCH(k_huff_scan, dim3(segs), dim3(jpeg::HUFF_WG), 0, st, base, pages, npages);
  RT_LAUNCH(k_huff_write, dim3(wgs), dim3(jpeg::HUFF_WG), 0, st, base, pages, npages, info);
  RT_LAUNCH(k_huff_dc, dim3(segs * 3), dim3(jpeg::HUFF_WG), 0, st, base, pages, npages, info);
}

}  // namespace rt
