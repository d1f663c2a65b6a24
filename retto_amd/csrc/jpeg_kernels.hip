// JPEG pixel reconstruction on gfx950 for the pages of one lane part (rt_submit_encoded_batch, rt_decode_batch): the host has
// entropy-decoded each page into quantised int16 coefficients; k_jpeg_idct dequantises and inverse-transforms every 8x8 block
// into the page's MCU-padded component planes, k_jpeg_color upsamples the chroma planes and writes interleaved RGB8.  The
// arithmetic is jpeg_recon.h's, shared with the host check; integer-only, bit-identical to JpegDec (image_decode.cpp).
#include "common.h"
#include "jpeg_recon.h"

namespace rt {
namespace {

constexpr int IDCT_BLOCKS = 32;   // 8x8 blocks per 256-thread workgroup: 8 lanes per block
constexpr int WS_LD = 9;          // LDS row pitch of the pass-1 result (ints): pass-2 lanes read rows 9 banks apart

// the last component whose first block is <= g (comps sorted by block_base; the first one starts at 0)
__device__ inline int find_comp(const jpeg::DevComp* comps, int ncomps, int g) {
  int lo = 0, hi = ncomps - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (comps[mid].block_base <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// lane (block jb = tid / 8, c = tid % 8): column c in pass 1, row c in pass 2; one 8-byte store per output row
__global__ __launch_bounds__(256) void k_jpeg_idct(uint8_t* __restrict__ base, const jpeg::DevComp* __restrict__ comps,
                                                   int ncomps, int total_blocks) {
  __shared__ int ws[IDCT_BLOCKS][8 * WS_LD];
  const int jb = threadIdx.x >> 3, c = threadIdx.x & 7;
  const int g = blockIdx.x * IDCT_BLOCKS + jb;
  const bool live = g < total_blocks;
  const jpeg::DevComp* cm = nullptr;
  int b = 0;
  if (live) {
    cm = comps + find_comp(comps, ncomps, g);
    b = g - cm->block_base;
    const int16_t* blk = (const int16_t*)(base + cm->coef_off) + (size_t)b * 64;
    jpeg::idct_col(blk, cm->q, c, ws[jb], WS_LD);
  }
  __syncthreads();
  if (live) {
    alignas(8) uint8_t o[8];
    jpeg::idct_row(ws[jb] + c * WS_LD, o);
    const int by = b / cm->blocks_w, bx = b - by * cm->blocks_w;
    // stride is a multiple of 8 and plane_off of 256: the store is 8-byte aligned
    uint8_t* dst = base + cm->plane_off + (size_t)(by * 8 + c) * cm->stride + (size_t)bx * 8;
    *(uint64_t*)dst = *(const uint64_t*)o;
  }
}

__device__ inline int find_page(const jpeg::DevPage* pages, int npages, int64_t gi) {
  int lo = 0, hi = npages - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pages[mid].pix_base <= gi) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// one thread per output pixel (grid-stride): grey replication, RGB-coded pass-through or jdcolor YCbCr -> RGB
__global__ __launch_bounds__(256) void k_jpeg_color(uint8_t* __restrict__ base, const jpeg::DevComp* __restrict__ comps,
                                                    const jpeg::DevPage* __restrict__ pages, int npages, int64_t total) {
  for (int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gi < total; gi += (int64_t)gridDim.x * blockDim.x) {
    const jpeg::DevPage& P = pages[find_page(pages, npages, gi)];
    const int64_t p = gi - P.pix_base;
    const int y = (int)(p / P.W), x = (int)(p - (int64_t)y * P.W);
    uint8_t* o = base + P.rgb_off + (size_t)p * 3;
    if (P.nc == 1) {
      const jpeg::DevComp& C0 = comps[P.comp[0]];
      o[0] = o[1] = o[2] = base[C0.plane_off + (size_t)y * C0.stride + x];
      continue;
    }
    uint8_t v[3];
    for (int i = 0; i < 3; i++) {
      const jpeg::DevComp& C = comps[P.comp[i]];
      v[i] = jpeg::up_sample(base + C.plane_off, C.stride, C.cw, C.ch, C.fh, C.fv, x, y);
    }
    if (P.is_rgb) { o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; }
    else jpeg::ycc_rgb(v[0], v[1], v[2], o);
  }
}

}  // namespace

void launch_jpeg_idct(uint8_t* base, const jpeg::DevComp* comps, int ncomps, int total_blocks, hipStream_t st) {
  if (total_blocks <= 0) return;
  RT_LAUNCH(k_jpeg_idct, dim3((total_blocks + IDCT_BLOCKS - 1) / IDCT_BLOCKS), dim3(256), 0, st, base, comps, ncomps,
            total_blocks);
}
void launch_jpeg_color(uint8_t* base, const jpeg::DevComp* comps, const jpeg::DevPage* pages, int npages, int64_t total_pixels,
                       hipStream_t st) {
  if (total_pixels <= 0) return;
  const int64_t want = (total_pixels + 255) / 256;
  const int grid = (int)(want < 16384 ? want : 16384);
  RT_LAUNCH(k_jpeg_color, dim3(grid), dim3(256), 0, st, base, comps, pages, npages, total_pixels);
}

}  // namespace rt
