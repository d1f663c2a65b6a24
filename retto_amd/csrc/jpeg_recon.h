// JPEG pixel reconstruction shared by the host check (rt_debug_jpeg_reconstruct) and the gfx950 kernels
// (jpeg_kernels.hip): dequantisation, the jidctint "islow" inverse DCT and the per-pixel chroma upsampling / colour conversion,
// written once as __host__ __device__ functions.  Every function restates JpegDec (image_decode.cpp) operation for operation:
// idct_store, decode_block / finish_progressive's clamp, upsample() and the colour loop of run().  The kernels add only their
// thread mapping on top, so a CPU build of these functions is the device arithmetic.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rt {
namespace jpeg {

// One page component as the kernels see it.  Offsets are in bytes from the page slot's base (coefficients: int16, block raster
// order over the MCU-padded plane, natural order inside a block; plane: stride x rows bytes).
struct DevComp {
  uint64_t coef_off, plane_off;
  int blocks_w, nblocks;   // blocks per plane row (stride / 8), blocks in the plane
  int block_base;          // first block of this component in the launch (prefix sum over the launch's components)
  int stride, cw, ch;      // plane row pitch, real sample size (upsample clamps rows to ch - 1)
  int fh, fv;              // hmax / hs, vmax / vs
  uint16_t q[64];          // quantisation table, natural order
};
// One page: three components (nc == 3) or one (grey), output RGB8 [H][W][3] at rgb_off.
struct DevPage {
  uint64_t rgb_off;
  int64_t pix_base;        // first pixel of this page in the launch (prefix sum over the launch's pages)
  int W, H, nc, is_rgb;
  int comp[3];             // indices into the launch's DevComp table
};

// decode_block / finish_progressive: coefficient * quantiser, clamped to +-2^24 (corrupt streams)
__host__ __device__ inline int dequant(int c, int q) {
  const int64_t v = (int64_t)c * q;
  return (int)(v < -(1LL << 24) ? -(1LL << 24) : v > (1LL << 24) ? (1LL << 24) : v);
}
__host__ __device__ inline int descale(int64_t x, int s) { return (int)((x + (1LL << (s - 1))) >> s); }

constexpr int CB = 13, P1 = 2;
constexpr int F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299,
              F1847 = 15137, F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;

// Pass 1 of idct_store for column `col` of one block: dequantises the column's 8 coefficients (blk: int16, natural order) and
// writes ws[col + ld * r], r = 0..7 (ld = 8 on the host; the kernel pads its LDS rows).  64-bit intermediates and the (int)
// narrowing of descale, as the host writes them.
__host__ __device__ inline void idct_col(const int16_t* blk, const uint16_t* q, int col, int* ws, int ld) {
  int p[8];
  for (int r = 0; r < 8; r++) p[r] = dequant(blk[8 * r + col], q[8 * r + col]);
  int64_t z2 = p[2], z3 = p[6];
  int64_t z1 = (z2 + z3) * F0541;
  int64_t t2 = z1 + z3 * (-F1847), t3 = z1 + z2 * F0765;
  z2 = p[0]; z3 = p[4];
  int64_t t0 = (z2 + z3) * (1LL << CB), t1 = (z2 - z3) * (1LL << CB);
  const int64_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  t0 = p[7]; t1 = p[5]; t2 = p[3]; t3 = p[1];
  z1 = t0 + t3; z2 = t1 + t2; z3 = t0 + t2; int64_t z4 = t1 + t3;
  const int64_t z5 = (z3 + z4) * F1175;
  t0 *= F0298; t1 *= F2053; t2 *= F3072; t3 *= F1501;
  z1 *= -F0899; z2 *= -F2562; z3 *= -F1961; z4 *= -F0390;
  z3 += z5; z4 += z5;
  t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
  int* w = ws + col;
  w[0] = descale(t10 + t3, CB - P1); w[7 * ld] = descale(t10 - t3, CB - P1);
  w[ld] = descale(t11 + t2, CB - P1); w[6 * ld] = descale(t11 - t2, CB - P1);
  w[2 * ld] = descale(t12 + t1, CB - P1); w[5 * ld] = descale(t12 - t1, CB - P1);
  w[3 * ld] = descale(t13 + t0, CB - P1); w[4 * ld] = descale(t13 - t0, CB - P1);
}
__host__ __device__ inline uint8_t idct_lim(int64_t x) {
  const int v = descale(x, CB + P1 + 3) + 128;
  return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}
// Pass 2 for one row: p = ws + ld * row -> o[0..7].  (A DC-only block gives (4 * dc + 16) >> 5 + 128 here, which is the host's
// flat-block shortcut, so the kernels always run the full transform.)
__host__ __device__ inline void idct_row(const int* p, uint8_t* o) {
  int64_t z2 = p[2], z3 = p[6];
  int64_t z1 = (z2 + z3) * F0541;
  int64_t t2 = z1 + z3 * (-F1847), t3 = z1 + z2 * F0765;
  int64_t t0 = ((int64_t)p[0] + p[4]) * (1LL << CB), t1 = ((int64_t)p[0] - p[4]) * (1LL << CB);
  const int64_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  t0 = p[7]; t1 = p[5]; t2 = p[3]; t3 = p[1];
  z1 = t0 + t3; z2 = t1 + t2; z3 = t0 + t2; int64_t z4 = t1 + t3;
  const int64_t z5 = (z3 + z4) * F1175;
  t0 *= F0298; t1 *= F2053; t2 *= F3072; t3 *= F1501;
  z1 *= -F0899; z2 *= -F2562; z3 *= -F1961; z4 *= -F0390;
  z3 += z5; z4 += z5;
  t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
  o[0] = idct_lim(t10 + t3); o[7] = idct_lim(t10 - t3); o[1] = idct_lim(t11 + t2); o[6] = idct_lim(t11 - t2);
  o[2] = idct_lim(t12 + t1); o[5] = idct_lim(t12 - t1); o[3] = idct_lim(t13 + t0); o[4] = idct_lim(t13 - t0);
}

// upsample(): the full-resolution sample (x, y) of one component plane, branch for branch -- h1v1 copy, fancy h2v1 / h2v2
// (cw > 2 only), h1v2 with its 1 / 2 bias, replication for every other integer factor.  Rows clamp to ch - 1.
__host__ __device__ inline uint8_t up_sample(const uint8_t* plane, int stride, int cw, int ch, int fh, int fv, int x, int y) {
  auto row = [&](int r) { return plane + (size_t)(r < 0 ? 0 : r > ch - 1 ? ch - 1 : r) * stride; };
  if (fh == 1 && fv == 1) return row(y)[x];
  if (fh == 2 && fv == 1 && cw > 2) {
    const uint8_t* in = row(y);
    const int i = x >> 1;
    if (x & 1) return i == cw - 1 ? in[cw - 1] : (uint8_t)((in[i] * 3 + in[i + 1] + 2) >> 2);
    return i == 0 ? in[0] : (uint8_t)((in[i] * 3 + in[i - 1] + 1) >> 2);
  }
  if (fh == 2 && fv == 2 && cw > 2) {
    const int r = y >> 1;
    const uint8_t* in0 = row(r);
    const uint8_t* in1 = row((y & 1) ? r + 1 : r - 1);
    const int i = x >> 1;
    const int s = in0[i] * 3 + in1[i];
    if (x & 1) {
      if (i == cw - 1) return (uint8_t)((s * 4 + 7) >> 4);
      return (uint8_t)((s * 3 + in0[i + 1] * 3 + in1[i + 1] + 7) >> 4);
    }
    if (i == 0) return (uint8_t)((s * 4 + 8) >> 4);
    return (uint8_t)((s * 3 + in0[i - 1] * 3 + in1[i - 1] + 8) >> 4);
  }
  if (fh == 1 && fv == 2) {
    const int r = y >> 1, bias = (y & 1) ? 2 : 1;
    return (uint8_t)((row(r)[x] * 3 + row((y & 1) ? r + 1 : r - 1)[x] + bias) >> 2);
  }
  const int xs = x / fh;
  return row(y / fv)[xs < cw - 1 ? xs : cw - 1];
}

// run()'s colour loop: jdcolor 16-bit fixed point, FIX(x) = (int)(x * 65536 + 0.5), computed inline instead of from tables
__host__ __device__ inline uint8_t lim255(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }
__host__ __device__ inline void ycc_rgb(int yv, int cb, int cr, uint8_t* o) {
  const int64_t xr = cr - 128, xb = cb - 128;
  const int crr = (int)((91881LL * xr + 32768) >> 16), cbb = (int)((116130LL * xb + 32768) >> 16);
  const int64_t crg = -46802LL * xr, cbg = -22554LL * xb + 32768;
  o[0] = lim255(yv + crr);
  o[1] = lim255(yv + (int)((cbg + crg) >> 16));
  o[2] = lim255(yv + cbb);
}

// Sampling layouts the kernels reconstruct (and the tests cover): grey, or three components each at (fh, fv) in
// {(1,1), (2,1), (2,2)} -- Pillow's 4:4:4, 4:2:2 and 4:2:0.  Every other JPEG is decoded on the host.
__host__ __device__ inline bool layout_on_device(int nc, const int* fh, const int* fv) {
  if (nc == 1) return true;
  for (int i = 0; i < nc; i++)
    if (!((fh[i] == 1 && fv[i] == 1) || (fh[i] == 2 && fv[i] == 1) || (fh[i] == 2 && fv[i] == 2))) return false;
  return true;
}

}  // namespace jpeg

// jpeg_kernels.hip: each launch covers every page of one lane part.  base: the slot both tables' offsets refer to.
void launch_jpeg_idct(uint8_t* base, const jpeg::DevComp* comps, int ncomps, int total_blocks, hipStream_t st);
void launch_jpeg_color(uint8_t* base, const jpeg::DevComp* comps, const jpeg::DevPage* pages, int npages, int64_t total_pixels,
                       hipStream_t st);

}  // namespace rt
