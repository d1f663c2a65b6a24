// Pre/post-processing kernels (gfx950).  Integer / f32 / f64 arithmetic restating
// retto-core's processors and the third-party crates they call (image 0.25.6,
// imageproc 0.25.0, geo 0.30, Clipper 6.4.2 via geo-clipper).
// Compiled with -ffp-contract=off: results must be bit-identical to the CPU path the
// reference runs, so no expression may be fused or re-associated.
#include "prepost.h"

#include "geom_math.h"

namespace rt {
namespace pp {

typedef unsigned char u8;

// ===========================================================================
// thumbnail (image::imageops::thumbnail, RGB8)
// ===========================================================================
struct ThumbSrc { const u8* p; int h, w; };

__device__ __forceinline__ u8 numcast_u8(float v, int* err) {
  if (!(v > -1.0f && v < 256.0f)) { *err = 1; return 0; }
  return (u8)v;
}

// One output pixel (outx, outy) of thumbnail(src -> nw x nh); writes 3 channels to o[].
__device__ void thumb_pixel(const ThumbSrc& s, int nw, int nh, uint32_t outx, uint32_t outy, u8* o, int* err) {
  const uint32_t W = (uint32_t)s.w, H = (uint32_t)s.h;
  float x_ratio = (float)s.w / (float)nw;
  float y_ratio = (float)s.h / (float)nh;
  float bottomf = (float)outy * y_ratio;
  float topf = bottomf + y_ratio;
  uint32_t bottom = min(max(gm::f32_as_u32(ceilf(bottomf)), 0u), H - 1);
  uint32_t top = min(max(gm::f32_as_u32(ceilf(topf)), bottom), H);
  float leftf = (float)outx * x_ratio;
  float rightf = leftf + x_ratio;
  uint32_t left = min(max(gm::f32_as_u32(ceilf(leftf)), 0u), W - 1);
  uint32_t right = min(max(gm::f32_as_u32(ceilf(rightf)), left), W);
  auto px = [&](uint32_t x, uint32_t y, int c) -> uint32_t {
    if (x >= W || y >= H) { *err = 1; return 0u; }
    return (uint32_t)s.p[((size_t)y * W + x) * 3 + c];
  };
  if (bottom != top && left != right) {
    uint32_t n = (right - left) * (top - bottom);
    uint32_t rnd = n / 2;
    uint32_t s0 = 0, s1 = 0, s2 = 0;
    for (uint32_t y = bottom; y < top; y++) {
      const u8* row = s.p + ((size_t)y * W + left) * 3;
      for (uint32_t x = left; x < right; x++, row += 3) { s0 += row[0]; s1 += row[1]; s2 += row[2]; }
    }
    uint32_t v0 = (s0 + rnd) / n, v1 = (s1 + rnd) / n, v2 = (s2 + rnd) / n;
    o[0] = (u8)min(v0, 255u); o[1] = (u8)min(v1, 255u); o[2] = (u8)min(v2, 255u);
  } else if (bottom != top) {
    float fract = (gm::fract_f32(leftf) + gm::fract_f32(rightf)) / 2.0f;
    uint32_t l = right - 1;
    float fact_right = fract / (float)(top - bottom);
    float fact_left = (1.0f - fract) / (float)(top - bottom);
    for (int c = 0; c < 3; c++) {
      uint32_t sl = 0, sr = 0;
      for (uint32_t y = bottom; y < top; y++) { sl += px(l, y, c); sr += px(l + 1, y, c); }
      o[c] = numcast_u8(fact_left * (float)sl + fact_right * (float)sr, err);
    }
  } else if (left != right) {
    float fract = (gm::fract_f32(topf) + gm::fract_f32(bottomf)) / 2.0f;
    uint32_t b = top - 1;
    float fact_top = fract / (float)(right - left);
    float fact_bot = (1.0f - fract) / (float)(right - left);
    for (int c = 0; c < 3; c++) {
      uint32_t sb = 0, st = 0;
      for (uint32_t x = left; x < right; x++) { sb += px(x, b, c); st += px(x, b + 1, c); }
      o[c] = numcast_u8(fact_bot * (float)sb + fact_top * (float)st, err);
    }
  } else {
    float frac_v = (gm::fract_f32(topf) + gm::fract_f32(bottomf)) / 2.0f;
    float frac_h = (gm::fract_f32(leftf) + gm::fract_f32(rightf)) / 2.0f;
    uint32_t l = right - 1, b = top - 1;
    float fact_tr = frac_v * frac_h;
    float fact_tl = frac_v * (1.0f - frac_h);
    float fact_br = (1.0f - frac_v) * frac_h;
    float fact_bl = (1.0f - frac_v) * (1.0f - frac_h);
    for (int c = 0; c < 3; c++) {
      float k_bl = (float)px(l, b, c), k_tl = (float)px(l, b + 1, c);
      float k_br = (float)px(l + 1, b, c), k_tr = (float)px(l + 1, b + 1, c);
      o[c] = numcast_u8(fact_br * k_br + fact_tr * k_tr + fact_bl * k_bl + fact_tl * k_tl, err);
    }
  }
}

__global__ __launch_bounds__(256) void k_thumbnail(ThumbSrc s, u8* __restrict__ dst, int nh, int nw, int* err_flag) {
  long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long long)nh * nw) return;
  int err = 0;
  u8 o[3];
  thumb_pixel(s, nw, nh, (uint32_t)(p % nw), (uint32_t)(p / nw), o, &err);
  dst[p * 3] = o[0]; dst[p * 3 + 1] = o[1]; dst[p * 3 + 2] = o[2];
  if (err) atomicOr(err_flag, 1);
}

void thumbnail_rgb8(hipStream_t st, const uint8_t* src, int h, int w, uint8_t* dst, int nh, int nw, int* err_flag) {
  long long total = (long long)nh * nw;
  if (total <= 0) return;
  if (h == 0 || w == 0) { (void)hipMemsetAsync(dst, 0, (size_t)total * 3, st); return; }
  if (h == nh && w == nw) {  // ratio 1: every output pixel is the 1x1 block average = the pixel itself
    (void)hipMemcpyAsync(dst, src, (size_t)total * 3, hipMemcpyDeviceToDevice, st);
    return;
  }
  RT_LAUNCH(k_thumbnail, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, ThumbSrc{src, h, w}, dst, nh, nw,
                     err_flag);
}

// ===========================================================================
// det normalise
// ===========================================================================
struct Norm3 { float scale, mean[3], stdv[3]; };
__global__ __launch_bounds__(256) void k_det_normalize(const u8* __restrict__ rgb, long long npix, Norm3 nm, int layout,
                                                       float* __restrict__ out) {
  long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= npix) return;
  float v[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {  // channel c of BGR
    float x = (float)rgb[p * 3 + (2 - c)];
    v[c] = (x * nm.scale - nm.mean[c]) / nm.stdv[c];
  }
  if (layout == 0) {
    float4 o = make_float4(v[0], v[1], v[2], 0.0f);
    reinterpret_cast<float4*>(out)[p] = o;
  } else {
    out[p] = v[0]; out[npix + p] = v[1]; out[2 * npix + p] = v[2];
  }
}
void det_normalize(hipStream_t st, const uint8_t* rgb, int h, int w, float scale, const float* mean3,
                   const float* std3, int layout, float* out) {
  long long npix = (long long)h * w;
  if (npix <= 0) return;
  Norm3 nm; nm.scale = scale;
  for (int i = 0; i < 3; i++) { nm.mean[i] = mean3[i]; nm.stdv[i] = std3[i]; }
  RT_LAUNCH(k_det_normalize, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, rgb, npix, nm, layout, out);
}


// ===========================================================================
// crops: imageproc warp_into(Bicubic, default white) + rotate270
// ===========================================================================
__device__ __forceinline__ u8 clamp_u8_trunc(float x) {
  if (x < 255.0f) { if (x > 0.0f) return (u8)x; return 0; }
  return 255;
}
__device__ __forceinline__ float cubic(float p0, float p1, float p2, float p3, float x) {
  return p1 + 0.5f * x * (p2 - p0 + x * (2.0f * p0 - 5.0f * p1 + 4.0f * p2 - p3 + x * (3.0f * (p1 - p2) + p3 - p0)));
}
// one output pixel p (row-major, pre-rotation dims) of crop d: the whole per-pixel rule -- bicubic taps, white outside the source,
// clamp_u8_trunc, the rotate270 store.  k_warp_crops and k_warp_crops_flat differ only in how a thread finds (d, p).
__device__ __forceinline__ void warp_pixel(const CropDesc& d, int p, u8* __restrict__ pool) {
  int y = p / d.w, x = p % d.w;
  float fx = (float)x, fy = (float)y;
  float dd = d.inv[6] * fx + d.inv[7] * fy + d.inv[8];
  float px = (d.inv[0] * fx + d.inv[1] * fy + d.inv[2]) / dd;
  float py = (d.inv[3] * fx + d.inv[4] * fy + d.inv[5]) / dd;
  u8 o[3] = {255, 255, 255};
  float left = floorf(px) - 1.0f, right = left + 4.0f;
  float top = floorf(py) - 1.0f, bottom = top + 4.0f;
  float xw = px - (left + 1.0f), yw = py - (top + 1.0f);
  if ((left >= 0.0f) && (right < (float)d.sw) && (top >= 0.0f) && (bottom < (float)d.sh)) {
    uint32_t l = gm::f32_as_u32(left), tp = gm::f32_as_u32(top);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      u8 col[4];
#pragma unroll
      for (uint32_t r = 0; r < 4; r++) {
        const u8* row = d.src + ((size_t)(tp + r) * d.sw + l) * 3 + c;
        col[r] = clamp_u8_trunc(cubic((float)row[0], (float)row[3], (float)row[6], (float)row[9], xw));
      }
      o[c] = clamp_u8_trunc(cubic((float)col[0], (float)col[1], (float)col[2], (float)col[3], yw));
    }
  }
  size_t dst;
  if (!d.rot) dst = (size_t)y * d.w + x;
  else dst = (size_t)(d.w - 1 - x) * d.h + y;  // rotate270: out(y, w-1-x) = in(x, y), out width = h
  u8* q = pool + d.out_off + dst * 3;
  q[0] = o[0]; q[1] = o[1]; q[2] = o[2];
}
__global__ __launch_bounds__(256) void k_warp_crops(const CropDesc* __restrict__ descs, u8* __restrict__ pool) {
  const CropDesc d = descs[blockIdx.y];
  int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= d.w * d.h) return;
  warp_pixel(d, p, pool);
}
void warp_crops(hipStream_t st, const CropDesc* descs, int n, int max_pix, uint8_t* pool) {
  if (n <= 0 || max_pix <= 0) return;
  for (int y0 = 0; y0 < n; y0 += RT_MAX_GRID_Y)  // one grid row per crop: chunked to the gridDim.y limit
    RT_LAUNCH(k_warp_crops, dim3((max_pix + 255) / 256, std::min(n - y0, RT_MAX_GRID_Y)), dim3(256), 0, st, descs + y0, pool);
}

// The same crops as one flat list of output pixels: pixel g of the call belongs to the last crop whose pix_base <= g (pix_base
// is the host's prefix sum of w * h; every crop has at least one pixel, so the bases strictly increase).  The grid follows the
// total, not n x the largest crop: crops cut from an unshrunk page differ in size by orders of magnitude.
__device__ inline int find_crop(const CropDesc* descs, int n, long long g) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].pix_base <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}
__global__ __launch_bounds__(256) void k_warp_crops_flat(const CropDesc* __restrict__ descs, int n, long long total,
                                                         u8* __restrict__ pool) {
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long long)gridDim.x * 256) {
    const CropDesc& d = descs[find_crop(descs, n, g)];
    const long long p = g - d.pix_base;
    if (p >= (long long)d.w * d.h) continue;   // (a descriptor table whose bases do not match its sizes writes nothing)
    warp_pixel(d, (int)p, pool);
  }
}
void warp_crops_flat(hipStream_t st, const CropDesc* descs, int n, long long total_pix, uint8_t* pool) {
  if (n <= 0 || total_pix <= 0) return;
  const long long want = (total_pix + 255) / 256;
  const int grid = (int)std::min<long long>(want, WARP_FLAT_MAX_BLOCKS);
  RT_LAUNCH(k_warp_crops_flat, dim3(grid), dim3(256), 0, st, descs, n, total_pix, pool);
}

// cls_processor.rs:108-121 (first-max argmax) + :163-166 rotate_180_in_place
__global__ __launch_bounds__(256) void k_cls_post_rotate(const float* __restrict__ probs, const int* __restrict__ crop_of_row,
                                                         float thresh, const CropRef* __restrict__ crops,
                                                         u8* __restrict__ pool, int* __restrict__ label_idx,
                                                         float* __restrict__ score) {
  int row = blockIdx.y;
  int ci = crop_of_row[row];
  float p0 = probs[row * 2], p1 = probs[row * 2 + 1];
  int idx = p1 > p0 ? 1 : 0;
  float sc = idx ? p1 : p0;
  if (blockIdx.x == 0 && threadIdx.x == 0) { label_idx[ci] = idx; score[ci] = sc; }
  if (!(idx == 1 && sc >= thresh)) return;
  const CropRef c = crops[ci];
  long long n = (long long)c.h * c.w;
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n / 2) return;
  u8* a = pool + c.off + i * 3;
  u8* b = pool + c.off + (n - 1 - i) * 3;
  u8 t0 = a[0], t1 = a[1], t2 = a[2];
  a[0] = b[0]; a[1] = b[1]; a[2] = b[2];
  b[0] = t0; b[1] = t1; b[2] = t2;
}
void cls_post_rotate(hipStream_t st, const float* probs, const int* crop_of_row, int rows, float thresh,
                     const CropRef* crops, uint8_t* pool, int max_pix, int* label_idx, float* score) {
  if (rows <= 0) return;
  int bx = std::max(1, (max_pix / 2 + 255) / 256);
  for (int y0 = 0; y0 < rows; y0 += RT_MAX_GRID_Y)
    RT_LAUNCH(k_cls_post_rotate, dim3(bx, std::min(rows - y0, RT_MAX_GRID_Y)), dim3(256), 0, st, probs + 2 * (size_t)y0,
              crop_of_row + y0, thresh, crops, pool, label_idx, score);
}

// image_helper.rs:176-209
__global__ __launch_bounds__(256) void k_resize_norm(const LineDesc* __restrict__ lines, int img_h, const u8* __restrict__ pool,
                                                     int layout, float* __restrict__ out, int* err_flag) {
  const LineDesc L = lines[blockIdx.y];
  long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long long)img_h * L.W) return;
  int y = (int)(p / L.W), x = (int)(p % L.W);
  float v[3] = {0.0f, 0.0f, 0.0f};
  if (x < L.resized_w) {
    int err = 0;
    u8 o[3];
    thumb_pixel(ThumbSrc{pool + L.crop_off, L.h, L.w}, L.resized_w, img_h, (uint32_t)x, (uint32_t)y, o, &err);
    if (err) atomicOr(err_flag, 1);
#pragma unroll
    for (int c = 0; c < 3; c++) { float t = (float)o[c] / 255.0f; v[c] = (t - 0.5f) / 0.5f; }
  }
  if (layout == 0) {
    reinterpret_cast<float4*>(out + L.out_off)[p] = make_float4(v[0], v[1], v[2], 0.0f);
  } else {
    long long plane = (long long)img_h * L.W;
    float* o = out + L.out_off;
    o[p] = v[0]; o[plane + p] = v[1]; o[2 * plane + p] = v[2];
  }
}
void resize_norm(hipStream_t st, const LineDesc* lines, int n, int img_h, int max_W, const uint8_t* pool, int layout,
                 float* out, int* err_flag) {
  if (n <= 0 || max_W <= 0) return;
  long long total = (long long)img_h * max_W;
  for (int y0 = 0; y0 < n; y0 += RT_MAX_GRID_Y)
    RT_LAUNCH(k_resize_norm, dim3((unsigned)((total + 255) / 256), std::min(n - y0, RT_MAX_GRID_Y)), dim3(256), 0, st,
              lines + y0, img_h, pool, layout, out, err_flag);
}

// rec_processor.rs:48-97
__global__ __launch_bounds__(64) void k_ctc_decode(const int* __restrict__ idx, const float* __restrict__ prob,
                                                   const ImgGeom* __restrict__ lines, int n, int* __restrict__ tokens,
                                                   int* __restrict__ n_tokens, float* __restrict__ score) {
  int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const ImgGeom g = lines[i];
  int T = g.H * g.W;
  int cnt = 0; float acc = 0.0f;
  for (int t = 0; t < T; t++) {
    int id = idx[g.off + t];
    bool sel = id != 0;
    if (t >= 1) sel = sel && id != idx[g.off + t - 1];
    if (sel) { tokens[g.off + cnt] = id; acc = acc + prob[g.off + t]; cnt++; }
  }
  n_tokens[i] = cnt;
  score[i] = acc / (float)(unsigned)cnt;
}
void ctc_decode(hipStream_t st, const int* idx, const float* prob, const ImgGeom* lines, int n, int* tokens,
                int* n_tokens, float* score) {
  if (n <= 0) return;
  RT_LAUNCH(k_ctc_decode, dim3((n + 63) / 64), dim3(64), 0, st, idx, prob, lines, n, tokens, n_tokens, score);
}

// rt_config.rec_return_word_box (word_boxes.h).  One wave64 per line: the kept columns (the selection k_ctc_decode makes) are
// compacted 64 time steps at a time with a ballot and a popcount prefix; then lane 0 runs the header's segmentation and
// geometry, which is serial in token order (the CJK pitch is an f32 sum in run order).
__global__ __launch_bounds__(64) void k_word_boxes(const int* __restrict__ idx, const int* __restrict__ tokens,
                                                   const int* __restrict__ n_tokens, const int* __restrict__ label,
                                                   const float* __restrict__ cls_score, float thresh,
                                                   const int* __restrict__ flip, const u8* __restrict__ raw_of_id,
                                                   const WordLineDesc* __restrict__ lines,
                                                   int* __restrict__ cols, int* __restrict__ n_words, wb::Word* __restrict__ words) {
  const int line = blockIdx.x, lane = threadIdx.x;
  const WordLineDesc d = lines[line];
  const int* id = idx + d.tok_off;
  int* col = cols + d.tok_off;
  int kept = 0;
  for (int t0 = 0; t0 < d.g.T; t0 += 64) {
    const int t = t0 + lane;
    bool sel = false;
    if (t < d.g.T) { const int v = id[t]; sel = v != 0 && (t == 0 || v != id[t - 1]); }
    const unsigned long long m = __ballot(sel);
    if (sel) col[kept + __popcll(m & ((1ull << lane) - 1ull))] = t;
    kept += __popcll(m);
  }
  __syncthreads();   // the columns other lanes wrote, for lane 0
  if (lane != 0) return;
  const int n = min(kept, n_tokens[line]);   // (equal: the same selection)
  // (rec flip, rec_flip.h: a line whose view 1 was taken is the other way up than the classifier left it; flip null = off)
  const int rot180 = rf::rot180(label[line] == 1 && cls_score[line] >= thresh, flip ? flip[line] : rf::ONE_WAY);
  n_words[line] = wb::line_words(raw_of_id, tokens + d.tok_off, col, n, d.g, rot180, words + d.tok_off);
}
void word_boxes(hipStream_t st, const int* idx, const int* tokens, const int* n_tokens, const int* label, const float* cls_score,
                float cls_thresh, const int* flip, const uint8_t* raw_of_id, const WordLineDesc* lines, int n, int* cols,
                int* n_words, wb::Word* words) {
  if (n <= 0) return;
  RT_LAUNCH(k_word_boxes, dim3(n), dim3(64), 0, st, idx, tokens, n_tokens, label, cls_score, cls_thresh, flip, raw_of_id, lines,
            cols, n_words, words);
}

// rt_config.rec_return_candidates (ctc_candidates.h).  One wave64 per line, the ballot / popcount-prefix compaction of
// k_word_boxes: kept token j of the line gets its time step and rank 0 at slot (line's first row + j).  With kept_row the line
// also appends its kept rows to the group's compact list, from the sum of the earlier lines' token counts (line order, so the
// list -- and with it every chunk of the logits recompute -- is the same on every run).
__global__ __launch_bounds__(64) void k_ctc_kept_rows(const int* __restrict__ idx, const float* __restrict__ prob,
                                                      const ImgGeom* __restrict__ lines, const int* __restrict__ n_tokens, int n,
                                                      int K, int* __restrict__ cols, cc::Cand* __restrict__ cands,
                                                      int* __restrict__ kept_row, int* __restrict__ kept_slot,
                                                      int* __restrict__ n_kept) {
  const int line = blockIdx.x, lane = threadIdx.x;
  const ImgGeom g = lines[line];
  const int T = g.H * g.W;
  int base = 0;
  if (kept_row) {
    for (int i = lane; i < line; i += 64) base += n_tokens[i];
    for (int o = 32; o >= 1; o >>= 1) base += __shfl_xor(base, o);
  }
  const int* id = idx + g.off;
  int cnt = 0;
  for (int t0 = 0; t0 < T; t0 += 64) {
    const int t = t0 + lane;
    bool sel = false; int v = 0;
    if (t < T) { v = id[t]; sel = cc::kept(v, t > 0 ? id[t - 1] : 0, t == 0); }
    const unsigned long long m = __ballot(sel);
    if (sel) {
      const int j = cnt + __popcll(m & ((1ull << lane) - 1ull));
      const long long slot = g.off + j;
      cols[slot] = t;
      cands[slot * K] = cc::Cand{v, prob[g.off + t]};
      if (kept_row) { kept_row[base + j] = (int)(g.off + t); kept_slot[base + j] = (int)slot; }
    }
    cnt += __popcll(m);
  }
  if (kept_row && line == n - 1 && lane == 0) *n_kept = base + cnt;
}
void ctc_kept_rows(hipStream_t st, const int* idx, const float* prob, const ImgGeom* lines, const int* n_tokens, int n, int K,
                   int* cols, cc::Cand* cands, int* kept_row, int* kept_slot, int* n_kept) {
  if (n <= 0) return;
  RT_LAUNCH(k_ctc_kept_rows, dim3(n), dim3(64), 0, st, idx, prob, lines, n_tokens, n, K, cols, cands, kept_row, kept_slot, n_kept);
}

__global__ __launch_bounds__(256) void k_ctc_gather_rows(const float4* __restrict__ z, int ld4, const int* __restrict__ kept_row,
                                                         int m, float4* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)m * ld4) return;
  const int r = (int)(i / ld4), c = (int)(i % ld4);
  out[i] = z[(long long)kept_row[r] * ld4 + c];
}
void ctc_gather_rows(hipStream_t st, const float* z, int ld, const int* kept_row, int m, float* out) {
  if (m <= 0) return;
  const long long n = (long long)m * (ld / 4);
  RT_LAUNCH(k_ctc_gather_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const float4*>(z), ld / 4,
            kept_row, m, reinterpret_cast<float4*>(out));
}

// One wave64 per kept row.  Pass 1: the lanes stream the row's logits as float4 (coalesced; the row pitch is a multiple of 4 and
// the GEMM's pad columns >= classes are masked out), each keeping its own best-first list of MAX_K - 1 classes other than the
// greedy one, and the row maximum.  Pass 2: sum(exp(l - max)) over every class (the row is 26 KB: it comes back from L2).  Then
// K - 1 rounds of a wave arg-max over the lanes' list heads (ties to the lower id); the lane that owned the winner pops it, lane r
// keeps round r's winner and writes rank r + 1.
// MASKED (ctc_charset.h): row i is time step kept_row[i] of the group, whose charset row_set[...] (0: none) limits the lists, the
// maximum and the sum to its classes; a disallowed column is skipped, never lowered.  MASKED = false is the kernel as it was.
template <bool MASKED>
__global__ __launch_bounds__(64) void k_ctc_topk(const float* __restrict__ logits, int ld, int classes,
                                                 const int* __restrict__ kept_slot, int m, int K, cc::Cand* __restrict__ cands,
                                                 const int* __restrict__ kept_row, const int* __restrict__ row_set,
                                                 const uint32_t* __restrict__ masks, int words) {
  constexpr int N = cc::MAX_K - 1;
  const int row = blockIdx.x, lane = threadIdx.x;
  if (row >= m) return;
  cc::Cand* out = cands + (long long)kept_slot[row] * K;
  const int tok = out[0].id;
  const float4* x = reinterpret_cast<const float4*>(logits + (long long)row * ld);
  const int nv = (classes + 3) / 4;
  const uint32_t* mask = nullptr;
  if (MASKED) { const int set = row_set[kept_row[row]]; if (set > 0) mask = masks + (long long)(set - 1) * words; }
  float L[N]; int I[N];
#pragma unroll
  for (int j = 0; j < N; j++) { L[j] = -INFINITY; I[j] = cc::EMPTY_ID; }
  float mx = -INFINITY;
  for (int v = lane; v < nv; v += 64) {
    const float4 q = x[v];
    const float e[4] = {q.x, q.y, q.z, q.w};
    const uint32_t bits = MASKED && mask ? cs::allowed4(mask, v) : 15u;
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int c = 4 * v + u;
      if (c < classes && (!MASKED || ((bits >> u) & 1u))) {
        mx = fmaxf(mx, e[u]);
        if (c != tok) cc::list_insert(L, I, e[u], c);
      }
    }
  }
  for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  float sum = 0.0f;
  for (int v = lane; v < nv; v += 64) {
    const float4 q = x[v];
    const float e[4] = {q.x, q.y, q.z, q.w};
    const uint32_t bits = MASKED && mask ? cs::allowed4(mask, v) : 15u;
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (4 * v + u < classes && (!MASKED || ((bits >> u) & 1u))) sum = sum + expf(e[u] - mx);
  }
  for (int o = 32; o >= 1; o >>= 1) sum = sum + __shfl_xor(sum, o);   // (a butterfly: every lane adds in the same order)
  float ol = 0.0f; int oi = cc::EMPTY_ID;
  for (int r = 0; r < K - 1; r++) {
    float wl = L[0]; int wi = I[0];
    for (int o = 32; o >= 1; o >>= 1) {
      const float l2 = __shfl_xor(wl, o); const int i2 = __shfl_xor(wi, o);
      if (cc::better(l2, i2, wl, wi)) { wl = l2; wi = i2; }
    }
    if (lane == r) { ol = wl; oi = wi; }
    if (wi != cc::EMPTY_ID && I[0] == wi) {
#pragma unroll
      for (int j = 0; j + 1 < N; j++) { L[j] = L[j + 1]; I[j] = I[j + 1]; }
      L[N - 1] = -INFINITY; I[N - 1] = cc::EMPTY_ID;
    }
  }
  if (lane < K - 1) out[1 + lane] = oi == cc::EMPTY_ID ? cc::Cand{-1, 0.0f} : cc::Cand{oi, cc::prob_of(ol, mx, sum)};
}
void ctc_topk(hipStream_t st, const float* logits, int ld, int classes, const int* kept_slot, int m, int K, cc::Cand* cands,
              const int* kept_row, const int* row_set, const uint32_t* masks, int words) {
  if (m <= 0 || K <= 1) return;
  if (masks && row_set && kept_row)
    RT_LAUNCH(k_ctc_topk<true>, dim3(m), dim3(64), 0, st, logits, ld, classes, kept_slot, m, K, cands, kept_row, row_set, masks, words);
  else
    RT_LAUNCH(k_ctc_topk<false>, dim3(m), dim3(64), 0, st, logits, ld, classes, kept_slot, m, K, cands, nullptr, nullptr, nullptr, 0);
}

// Rec charsets (ctc_charset.h).  One wave64 per restricted row i < m of logits [m][ld]: time step rows[i] of the group, whose
// charset is row_set[rows[i]] >= 1.  The lanes stream the row as float4; a lane's four columns lie in one mask word.  Pass 1: the
// maximum and its class over the allowed columns < classes, then a butterfly over (logit, id) with the tie rule, after which every
// lane holds the same pair.  Pass 2: sum(exp(l - max)) over the same columns (the row comes back from L2).  Lane 0 writes the
// row's idx and prob.
__global__ __launch_bounds__(64) void k_ctc_charset_argmax(const float* __restrict__ logits, int ld, int classes,
                                                           const int* __restrict__ rows, const int* __restrict__ row_set,
                                                           const uint32_t* __restrict__ masks, int words, int m,
                                                           int* __restrict__ idx, float* __restrict__ prob) {
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= m) return;
  const int row = rows[i], set = row_set[row];
  if (set <= 0) return;   // (never listed: a row of an unrestricted line keeps the fused head's values)
  const uint32_t* mask = masks + (long long)(set - 1) * words;
  const float4* x = reinterpret_cast<const float4*>(logits + (long long)i * ld);
  const int nv = (classes + 3) / 4;
  float bl = -INFINITY; int bi = cc::EMPTY_ID;
  for (int v = lane; v < nv; v += 64) {
    const float4 q = x[v];
    const float e[4] = {q.x, q.y, q.z, q.w};
    const uint32_t bits = cs::allowed4(mask, v);
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int c = 4 * v + u;
      if (c < classes && ((bits >> u) & 1u) && cc::better(e[u], c, bl, bi)) { bl = e[u]; bi = c; }
    }
  }
  for (int o = 32; o >= 1; o >>= 1) {
    const float l2 = __shfl_xor(bl, o); const int i2 = __shfl_xor(bi, o);
    if (cc::better(l2, i2, bl, bi)) { bl = l2; bi = i2; }
  }
  float sum = 0.0f;
  for (int v = lane; v < nv; v += 64) {
    const float4 q = x[v];
    const float e[4] = {q.x, q.y, q.z, q.w};
    const uint32_t bits = cs::allowed4(mask, v);
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (4 * v + u < classes && ((bits >> u) & 1u)) sum = sum + expf(e[u] - bl);
  }
  for (int o = 32; o >= 1; o >>= 1) sum = sum + __shfl_xor(sum, o);   // (a butterfly: every lane adds in the same order)
  if (lane == 0) { idx[row] = bi == cc::EMPTY_ID ? 0 : bi; prob[row] = cc::prob_of(bl, bl, sum); }   // (every allowed logit NaN: the blank)
}
void ctc_charset_argmax(hipStream_t st, const float* logits, int ld, int classes, const int* rows, const int* row_set,
                        const uint32_t* masks, int words, int m, int* idx, float* prob) {
  if (m <= 0) return;
  RT_LAUNCH(k_ctc_charset_argmax, dim3(m), dim3(64), 0, st, logits, ld, classes, rows, row_set, masks, words, m, idx, prob);
}

// Rec lexicons (ctc_lexicon.h).  One wave64 per row i < m of logits [m][ld]: lse[i] over the columns < classes, in the two-pass
// shape of k_ctc_charset_argmax (float4 streaming, pad columns skipped; the second pass comes back from L2).
__global__ __launch_bounds__(64) void k_ctc_row_lse(const float* __restrict__ logits, int ld, int classes, int m,
                                                    float* __restrict__ lse) {
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= m) return;
  const float4* x = reinterpret_cast<const float4*>(logits + (long long)i * ld);
  const int nv = (classes + 3) / 4;
  float mx = -INFINITY;
  for (int v = lane; v < nv; v += 64) {
    const float4 q = x[v];
    const float e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (4 * v + u < classes) mx = fmaxf(mx, e[u]);
  }
  for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  float sum = 0.0f;
  for (int v = lane; v < nv; v += 64) {
    const float4 q = x[v];
    const float e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (4 * v + u < classes) sum = sum + expf(e[u] - mx);
  }
  for (int o = 32; o >= 1; o >>= 1) sum = sum + __shfl_xor(sum, o);   // (a butterfly: every lane adds in the same order)
  if (lane == 0) lse[i] = lx::lse_of(mx, sum);
}
void ctc_row_lse(hipStream_t st, const float* logits, int ld, int classes, int m, float* lse) {
  if (m <= 0) return;
  RT_LAUNCH(k_ctc_row_lse, dim3(m), dim3(64), 0, st, logits, ld, classes, m, lse);
}

// The CTC forward recursion of a lexicon's entries over the lines of one chunk.  Workgroup (w, j) is one wave64: wave w of the
// lexicon of chunk line j.  A lexicon's waves go through its three buckets in turn (lx::waves_of): 4 entries of 16 lanes, 2 of
// 32, 1 of 64, each entry's states on the lanes of its group; waves past the lexicon's count (the grid is sized for the largest
// lexicon of the call) leave at once.  alpha lives in one register per lane; the neighbours' values come from __shfl_up within
// the group's width.  The T steps are a serial chain through expf / logf; the gathered logit l[t][cls(s)] and lse[t] do not
// depend on alpha, so they are loaded AHEAD steps early into a register ring (static indices: the loop is unrolled by AHEAD) and
// their latency hides behind the chain.  Every lane of the wave runs the same T steps -- a group without an entry (the partial
// last wave of a bucket) and the lanes past an entry's S states carry -inf along and read column 0 of the line's own rows -- so
// no shuffle is ever divergent; only lane 0 of a group that holds an entry writes, one float: loglik[line.out + entry].
__global__ __launch_bounds__(64) void k_ctc_lexicon_forward(const float* __restrict__ logits, int ld, const float* __restrict__ lse,
                                                            const lx::Line* __restrict__ lines, int chunk_row0,
                                                            const lx::Lex* __restrict__ lex, const lx::Entry* __restrict__ entries,
                                                            const int* __restrict__ order, const int* __restrict__ ids,
                                                            float* __restrict__ loglik) {
  constexpr int AHEAD = 4;
  const int lane = threadIdx.x;
  const lx::Line ln = lines[blockIdx.y];
  const lx::Lex X = lex[ln.lex];
  const int w16 = (X.n16 + 3) / 4, w32 = (X.n32 + 1) / 2, n64 = X.n - X.n16 - X.n32;
  int w = blockIdx.x, width, k, bucket_n, bucket_first;
  if (w < w16) { width = 16; k = 4 * w + (lane >> 4); bucket_n = X.n16; bucket_first = 0; }
  else if ((w -= w16) < w32) { width = 32; k = 2 * w + (lane >> 5); bucket_n = X.n32; bucket_first = X.n16; }
  else if ((w -= w32) < n64) { width = 64; k = w; bucket_n = n64; bucket_first = X.n16 + X.n32; }
  else return;
  const bool live = k < bucket_n;
  const int e = live ? order[X.first + bucket_first + k] : 0;   // (lexicon-local entry index)
  const lx::Entry E = live ? entries[X.first + e] : lx::Entry{0, 0, 0};
  const int s = lane & (width - 1), S = 2 * E.len + 1, T = ln.T;
  const bool mine = live && s < S;
  const int cls = mine ? lx::cls_of(ids + E.off, s) : 0;
  const bool skip = mine && lx::skip_of(ids + E.off, s);
  const float* col = logits + (long long)(ln.row0 - chunk_row0) * ld + cls;
  const float* ls = lse + (ln.row0 - chunk_row0);
  float lq[AHEAD], eq[AHEAD];
#pragma unroll
  for (int j = 0; j < AHEAD; j++) { lq[j] = j < T ? col[(long long)j * ld] : 0.0f; eq[j] = j < T ? ls[j] : 0.0f; }
  float a = -INFINITY;
  for (int t0 = 0; t0 < T; t0 += AHEAD) {
#pragma unroll
    for (int j = 0; j < AHEAD; j++) {
      const int t = t0 + j;
      if (t < T) {   // (wave-uniform)
        const float lp = lq[j] - eq[j];
        if (t + AHEAD < T) { lq[j] = col[(long long)(t + AHEAD) * ld]; eq[j] = ls[t + AHEAD]; }
        const float u1 = __shfl_up(a, 1, width), u2 = __shfl_up(a, 2, width);
        const float a1 = s >= 1 ? u1 : -INFINITY, a2 = s >= 2 ? u2 : -INFINITY;
        const float nx = t == 0 ? (s < 2 ? lp : -INFINITY) : lx::step(a, a1, a2, skip, lp);
        a = mine ? nx : -INFINITY;
      }
    }
  }
  const float f1 = __shfl(a, S - 1, width), f2 = __shfl(a, S >= 2 ? S - 2 : 0, width);
  if (live && s == 0) loglik[ln.out + e] = T >= E.need ? lx::lae(f1, f2, -INFINITY) : -INFINITY;
}
void ctc_lexicon_forward(hipStream_t st, const float* logits, int ld, const float* lse, const lx::Line* lines, int n_lines,
                         int chunk_row0, int max_waves, const lx::Lex* lex, const lx::Entry* entries, const int* order,
                         const int* ids, float* loglik) {
  if (n_lines <= 0 || max_waves <= 0) return;
  RT_LAUNCH(k_ctc_lexicon_forward, dim3(max_waves, n_lines), dim3(64), 0, st, logits, ld, lse, lines, chunk_row0, lex, entries,
            order, ids, loglik);
}

// One wave64 per lexicon line over its loglik row: each lane keeps a best-first list of MATCHES feasible entries (an infeasible
// entry, -inf, is skipped, never ranked) and the maximum; pass 2 sums exp(loglik - max) over the feasible entries, by the
// butterfly of k_ctc_topk; then MATCHES rounds of a wave arg-max over the list heads (ties to the lower entry index), lane r
// keeping round r's winner and writing match r.  Lane 0 writes the count.
__global__ __launch_bounds__(64) void k_ctc_lexicon_topk(const lx::Line* __restrict__ lines, const lx::Lex* __restrict__ lex,
                                                         const float* __restrict__ loglik, lx::Match* __restrict__ matches,
                                                         int* __restrict__ counts) {
  constexpr int N = lx::MATCHES;
  const int lane = threadIdx.x;
  const lx::Line ln = lines[blockIdx.x];
  const int n = lex[ln.lex].n;
  const float* x = loglik + ln.out;
  float L[N]; int I[N];
#pragma unroll
  for (int j = 0; j < N; j++) { L[j] = -INFINITY; I[j] = cc::EMPTY_ID; }
  float mx = -INFINITY;
  for (int e = lane; e < n; e += 64) {
    const float v = x[e];
    if (v > -INFINITY) { mx = fmaxf(mx, v); cc::list_insert(L, I, v, e); }
  }
  for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  float sum = 0.0f;
  for (int e = lane; e < n; e += 64) {
    const float v = x[e];
    if (v > -INFINITY) sum = sum + expf(v - mx);
  }
  for (int o = 32; o >= 1; o >>= 1) sum = sum + __shfl_xor(sum, o);   // (a butterfly: every lane adds in the same order)
  float ol = 0.0f; int oi = cc::EMPTY_ID, cnt = 0;
  for (int r = 0; r < N; r++) {
    float wl = L[0]; int wi = I[0];
    for (int o = 32; o >= 1; o >>= 1) {
      const float l2 = __shfl_xor(wl, o); const int i2 = __shfl_xor(wi, o);
      if (cc::better(l2, i2, wl, wi)) { wl = l2; wi = i2; }
    }
    if (lane == r) { ol = wl; oi = wi; }
    if (wi != cc::EMPTY_ID) cnt++;
    if (wi != cc::EMPTY_ID && I[0] == wi) {
#pragma unroll
      for (int j = 0; j + 1 < N; j++) { L[j] = L[j + 1]; I[j] = I[j + 1]; }
      L[N - 1] = -INFINITY; I[N - 1] = cc::EMPTY_ID;
    }
  }
  if (lane < N && oi != cc::EMPTY_ID) matches[(long long)ln.slot * N + lane] = lx::Match{oi, ol, lx::posterior_of(ol, mx, sum)};
  if (lane == 0) counts[ln.slot] = cnt;
}
void ctc_lexicon_topk(hipStream_t st, const lx::Line* lines, int n_lines, const lx::Lex* lex, const float* loglik,
                      lx::Match* matches, int* counts) {
  if (n_lines <= 0) return;
  RT_LAUNCH(k_ctc_lexicon_topk, dim3(n_lines), dim3(64), 0, st, lines, lex, loglik, matches, counts);
}

// Rec keywords (ctc_keyword.h): k_ctc_lexicon_forward's sibling.  Workgroup (w, j) is one wave64: wave w of the keyword list of
// chunk line j, through the list's three buckets in turn (4 entries of 16 lanes, 2 of 32, 1 of 64; an entry of L ids has 2 L - 1
// states, which fit the lexicon's widths); waves past the list's count leave at once.  One lane is one state: its (v, a) live in
// two registers and the neighbours' come from __shfl_up within the group's width.  The chain has no expf or logf: a step is two
// compares and one add; the gathered logit l[t][cls(s)] and rmax[t] do not depend on it and are loaded AHEAD steps early into a
// register ring (static indices: the loop is unrolled by AHEAD).  Every lane of the wave runs the same T steps -- a group
// without an entry and the lanes past an entry's states carry (-inf, -1) along and read column 0 of the line's own rows -- so
// no shuffle is ever divergent.  Every lane keeps the running end of its own state; the one of state 2 L - 2 is the entry's,
// and lane 0 of a group that holds an entry fetches it and writes score[line.out + entry] and the two int32 of its span.
__global__ __launch_bounds__(64) void k_ctc_keyword_spot(const float* __restrict__ logits, int ld, const float* __restrict__ rmax,
                                                         const kw::Line* __restrict__ lines, int chunk_row0,
                                                         const lx::Lex* __restrict__ lex, const lx::Entry* __restrict__ entries,
                                                         const int* __restrict__ order, const int* __restrict__ ids,
                                                         float* __restrict__ score, int* __restrict__ span) {
  constexpr int AHEAD = 4;
  const int lane = threadIdx.x;
  const kw::Line ln = lines[blockIdx.y];
  const lx::Lex X = lex[ln.lex];
  const int w16 = (X.n16 + 3) / 4, w32 = (X.n32 + 1) / 2, n64 = X.n - X.n16 - X.n32;
  int w = blockIdx.x, width, k, bucket_n, bucket_first;
  if (w < w16) { width = 16; k = 4 * w + (lane >> 4); bucket_n = X.n16; bucket_first = 0; }
  else if ((w -= w16) < w32) { width = 32; k = 2 * w + (lane >> 5); bucket_n = X.n32; bucket_first = X.n16; }
  else if ((w -= w32) < n64) { width = 64; k = w; bucket_n = n64; bucket_first = X.n16 + X.n32; }
  else return;
  const bool live = k < bucket_n;
  const int e = live ? order[X.first + bucket_first + k] : 0;   // (list-local entry index)
  const lx::Entry E = live ? entries[X.first + e] : lx::Entry{0, 1, 1};
  const int s = lane & (width - 1), S = 2 * E.len - 1, T = ln.T;
  const bool mine = live && s < S;
  const int cls = mine ? kw::cls_of(ids + E.off, s) : 0;
  const bool skip = mine && kw::skip_of(ids + E.off, s);
  const float* col = logits + (long long)(ln.row0 - chunk_row0) * ld + cls;
  const float* rm = rmax + (ln.row0 - chunk_row0);
  float lq[AHEAD], mq[AHEAD];
#pragma unroll
  for (int j = 0; j < AHEAD; j++) { lq[j] = j < T ? col[(long long)j * ld] : 0.0f; mq[j] = j < T ? rm[j] : 0.0f; }
  kw::Cell c{-INFINITY, -1};
  float best = -INFINITY; int first = -1, last = -1;
  for (int t0 = 0; t0 < T; t0 += AHEAD) {
#pragma unroll
    for (int j = 0; j < AHEAD; j++) {
      const int t = t0 + j;
      if (t < T) {   // (wave-uniform)
        const float d = lq[j] - mq[j];
        if (t + AHEAD < T) { lq[j] = col[(long long)(t + AHEAD) * ld]; mq[j] = rm[t + AHEAD]; }
        const kw::Cell p1{__shfl_up(c.v, 1, width), __shfl_up(c.a, 1, width)}, p2{__shfl_up(c.v, 2, width), __shfl_up(c.a, 2, width)};
        const kw::Cell nx = t == 0 ? (s == 0 ? kw::Cell{d, 0} : kw::Cell{-INFINITY, -1}) : kw::step(s, t, c, p1, p2, skip, d);
        c = mine ? nx : kw::Cell{-INFINITY, -1};
        if (c.v > best) { best = c.v; first = c.a; last = t; }
      }
    }
  }
  const float fs = __shfl(best, S - 1, width);
  const int ff = __shfl(first, S - 1, width), fl = __shfl(last, S - 1, width);
  if (live && s == 0) {
    const bool feasible = T >= E.need;
    score[ln.out + e] = feasible ? fs : -INFINITY;
    span[2 * (ln.out + e)] = feasible ? ff : -1; span[2 * (ln.out + e) + 1] = feasible ? fl : -1;
  }
}
void ctc_keyword_spot(hipStream_t st, const float* logits, int ld, const float* rmax, const kw::Line* lines, int n_lines,
                      int chunk_row0, int max_waves, const lx::Lex* lex, const lx::Entry* entries, const int* order, const int* ids,
                      float* score, int* span) {
  if (n_lines <= 0 || max_waves <= 0) return;
  RT_LAUNCH(k_ctc_keyword_spot, dim3(max_waves, n_lines), dim3(64), 0, st, logits, ld, rmax, lines, chunk_row0, lex, entries, order,
            ids, score, span);
}

// One wave64 per keyword line over its score row: each lane keeps a best-first list of kw::HITS entries that pass the list's
// min_score (kw::passes: never a -inf, never a NaN); then kw::HITS rounds of a wave arg-max over the list heads (ties to the
// lower entry index), lane r keeping round r's winner and writing hit r: entry, score and the span's two columns, never the
// quad.  Lane 0 writes the count.
__global__ __launch_bounds__(64) void k_ctc_keyword_topk(const kw::Line* __restrict__ lines, const lx::Lex* __restrict__ lex,
                                                         const float* __restrict__ min_score, const float* __restrict__ score,
                                                         const int* __restrict__ span, kw::Hit* __restrict__ hits,
                                                         int* __restrict__ counts) {
  constexpr int N = kw::HITS;
  const int lane = threadIdx.x;
  const kw::Line ln = lines[blockIdx.x];
  const int n = lex[ln.lex].n;
  const float floor_ = min_score[ln.lex];
  const float* x = score + ln.out;
  float L[N]; int I[N];
#pragma unroll
  for (int j = 0; j < N; j++) { L[j] = -INFINITY; I[j] = cc::EMPTY_ID; }
  for (int e = lane; e < n; e += 64) {
    const float v = x[e];
    if (kw::passes(v, floor_)) cc::list_insert(L, I, v, e);
  }
  float ol = 0.0f; int oi = cc::EMPTY_ID, cnt = 0;
  for (int r = 0; r < N; r++) {
    float wl = L[0]; int wi = I[0];
    for (int o = 32; o >= 1; o >>= 1) {
      const float l2 = __shfl_xor(wl, o); const int i2 = __shfl_xor(wi, o);
      if (cc::better(l2, i2, wl, wi)) { wl = l2; wi = i2; }
    }
    if (lane == r) { ol = wl; oi = wi; }
    if (wi != cc::EMPTY_ID) cnt++;
    if (wi != cc::EMPTY_ID && I[0] == wi) {
#pragma unroll
      for (int j = 0; j + 1 < N; j++) { L[j] = L[j + 1]; I[j] = I[j + 1]; }
      L[N - 1] = -INFINITY; I[N - 1] = cc::EMPTY_ID;
    }
  }
  if (lane < N && oi != cc::EMPTY_ID) {
    kw::Hit& h = hits[(long long)ln.slot * N + lane];
    h.entry = oi; h.score = ol; h.first_col = span[2 * (ln.out + oi)]; h.last_col = span[2 * (ln.out + oi) + 1];
  }
  if (lane == 0) counts[ln.slot] = cnt;
}
void ctc_keyword_topk(hipStream_t st, const kw::Line* lines, int n_lines, const lx::Lex* lex, const float* min_score,
                      const float* score, const int* span, kw::Hit* hits, int* counts) {
  if (n_lines <= 0) return;
  RT_LAUNCH(k_ctc_keyword_topk, dim3(n_lines), dim3(64), 0, st, lines, lex, min_score, score, span, hits, counts);
}

// Rec beams (ctc_beam.h).  One wave64 per row i < m of logits [m][ld]: K_t, the up to bm::TOP_C non-blank classes with the largest
// logits, in k_ctc_topk's shape -- the lanes stream the row once as float4 (pad columns and the blank skipped), each keeping a
// best-first list of TOP_C; then TOP_C rounds of a wave arg-max over the list heads (ties to the lower id), lane r keeping round
// r's winner and writing slot r: (cc::EMPTY_ID, -inf) past the row's count.  The beam kernel then never reads a whole row.
__global__ __launch_bounds__(64) void k_ctc_beam_topc(const float* __restrict__ logits, int ld, int classes, int m,
                                                      bm::TopC* __restrict__ topc) {
  constexpr int N = bm::TOP_C;
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= m) return;
  const float4* x = reinterpret_cast<const float4*>(logits + (long long)i * ld);
  const int nv = (classes + 3) / 4;
  float L[N]; int I[N];
#pragma unroll
  for (int j = 0; j < N; j++) { L[j] = -INFINITY; I[j] = cc::EMPTY_ID; }
  for (int v = lane; v < nv; v += 64) {
    const float4 q = x[v];
    const float e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int c = 4 * v + u;
      if (c >= 1 && c < classes) cc::list_insert(L, I, e[u], c);
    }
  }
  float ol = -INFINITY; int oi = cc::EMPTY_ID;
  for (int r = 0; r < N; r++) {
    float wl = L[0]; int wi = I[0];
    for (int o = 32; o >= 1; o >>= 1) {
      const float l2 = __shfl_xor(wl, o); const int i2 = __shfl_xor(wi, o);
      if (cc::better(l2, i2, wl, wi)) { wl = l2; wi = i2; }
    }
    if (lane == r) { ol = wl; oi = wi; }
    if (wi != cc::EMPTY_ID && I[0] == wi) {
#pragma unroll
      for (int j = 0; j + 1 < N; j++) { L[j] = L[j + 1]; I[j] = I[j + 1]; }
      L[N - 1] = -INFINITY; I[N - 1] = cc::EMPTY_ID;
    }
  }
  if (lane < N) { topc[i].id[lane] = oi; topc[i].logit[lane] = oi == cc::EMPTY_ID ? -INFINITY : ol; }
}
void ctc_beam_topc(hipStream_t st, const float* logits, int ld, int classes, int m, bm::TopC* topc) {
  if (m <= 0) return;
  RT_LAUNCH(k_ctc_beam_topc, dim3(m), dim3(64), 0, st, logits, ld, classes, m, topc);
}

// The prefix beam search of one chunk's lines: one workgroup of MAX_BEAM * TOP_C = 256 threads per line, T steps in sequence.
// The beam -- per member its trie node, that node's parent, its last class, its length, pb and pnb -- lives in LDS twice (this
// step's and the next's); so do the members' totals, the stay values and the totals of the step's bm::CANDS candidates.  Thread
// (j, r) = (tid / TOP_C, tid % TOP_C) owns ext_{j,r}; thread j < MAX_BEAM also owns stay_j.  A step, between barriers:
//   A  thread j: total_j, stay_j's pb' and pnb' (one gathered logit: l[t][last_j]); every thread: its class of K_t;
//   B  thread (j, r): its pnb'; a scan of the beam for the member that IS string_j + c (parent == node_j && last == c): found,
//      it folds its value into that member's stay pnb' -- the only thread that can (ctc_beam.h "merge") -- and has no candidate;
//   C  thread j: stay_j's total;
//   D  every candidate counts the candidates that rank before it (cc::better over the totals in LDS, broadcast reads): that
//      number is its place in the new beam, B or more: it is out.  No sort, no atomics, and the rule's total order to the bit.
//      A surviving extension then looks its string up among its parent's children (read only);
//   E  ... and, not found, creates node 1 + t B + place (no counter: the place is unique) and pushes it onto its parent's list
//      with one atomic exchange of the head; the survivors write the next beam, whose size is the largest place + 1.
// The trie is in global memory (ctc_beam.h "Device form"): what one step writes the next reads behind a barrier, within one
// workgroup.  At the end thread k < N walks hypothesis k's nodes to the root and writes its tokens back to front.
// Bounds: a row index is < the chunk's rows (a line's rows are resident together), a node id <= T B < bm::nodes_of(T, B), a
// token slot < N T.
// LM: language-model fusion (ctc_lm.h), a compile-time variant; LM = false is the kernel as it was, to the bit.  A member's model
// state and lm live in LDS twice, like pb and pnb; the candidates' keys (lm::key_of) beside their totals.  In B thread (j, r),
// where its extension is a candidate, looks its class up from state_j (lm::step): at the unigram level one indexed load of the
// dense table, above it one binary search per back-off level; the tables are read-only global memory.  D ranks by the key, E
// writes the survivors' state and lm; the trie is untouched.  Bounds: lm::step reads state s only for 0 < s < n_states (anything
// else is the empty context), cuts a state's arc slice to [0, n_arcs) and searches inside it in at most lm::ARC_STEPS halvings,
// walks at most lm::MAX_ORDER levels, and reads uni[c] only for 1 <= c < classes; a record slot < n_lines nbest as beams'.
// VC: the word-list constraint (ctc_vocab.h), a second compile-time switch; the instances without it are the kernel as it was, to
// the bit.  A member's trie state and its count of words that are no entries live in LDS twice beside state and lm; the
// candidates have keys (vc::key_of over the fused score with LM, over the total without).  In B thread (j, r) takes vc::step
// from vstate_j BEFORE it scans the beam for its merge target: the lookup -- one mask word, then one indexed load of the root's
// dense table or one node record and a binary search of its arc slice -- needs only what the last barrier published, so its
// loads are in flight under the scan and not behind it.  C gives the stays their keys, D ranks by the key, E writes the
// survivors' vstate and count.  After the last step a closing phase: thread j < n takes its closing key (the count plus
// vc::close of its state), counts the members that rank before it (the same counting selection: no sort, no atomics) and, if
// its place is below nbest, writes its record, its rt_beam_vocab and its tokens there.  The tables are read-only global memory.
// Bounds: vc::step reads mask[c >> 5] and root[c] only for 1 <= c < classes, node s only for 0 < s < n_nodes (anything else is
// OFF), cuts a node's arc slice to [0, n_arcs) and searches inside it in at most vc::ARC_STEPS halvings; vc::close reads node s
// only for 0 < s < n_nodes; a closing place is < n <= B, written only below nbest: a record slot < n_lines nbest as beams'.
template <bool LM, bool VC>
__global__ __launch_bounds__(256) void k_ctc_beam_search(const float* __restrict__ logits, int ld, const float* __restrict__ lse,
                                                         const bm::TopC* __restrict__ topc, const bm::Line* __restrict__ lines,
                                                         int chunk_row0, int B, int nbest, bm::Node* nodes,
                                                         bm::Beam* __restrict__ beams, int* __restrict__ tokens,
                                                         int* __restrict__ counts, lm::Fusion fu, lm::BeamLm* __restrict__ lms,
                                                         vc::Constraint wc, vc::BeamVocab* __restrict__ vocs) {
  constexpr int MB = bm::MAX_BEAM, TC = bm::TOP_C;
  static_assert(MB * TC == 256 && bm::CANDS == MB + 256, "one thread per extension");
  __shared__ int s_node[2][MB], s_par[2][MB], s_last[2][MB], s_len[2][MB], s_n[2];
  __shared__ float s_pb[2][MB], s_pnb[2][MB], s_tot[MB], s_spb[MB], s_spnb[MB], s_cand[bm::CANDS];
  __shared__ int s_state[2][LM ? MB : 1];
  __shared__ float s_lm[2][LM ? MB : 1], s_key[LM || VC ? bm::CANDS : 1];
  __shared__ int s_vstate[2][VC ? MB : 1], s_oov[2][VC ? MB : 1];
  const float* rank = LM || VC ? s_key : s_cand;   // what D orders by
  const int tid = threadIdx.x, j = tid / TC, r = tid % TC;
  const bm::Line ln = lines[blockIdx.x];
  const int T = ln.T;
  if (T <= 0) { if (tid == 0) counts[ln.slot] = 0; return; }   // (block-uniform)
  bm::Node* nd = nodes + ln.lex;
  const int n_nodes = (int)bm::nodes_of(T, B);
  const long long row0 = ln.row0 - chunk_row0;
  if (tid == 0) {
    nd[0] = bm::Node{-1, 0, -1, -1};
    s_node[0][0] = 0; s_par[0][0] = -1; s_last[0][0] = 0; s_len[0][0] = 0; s_pb[0][0] = 0.0f; s_pnb[0][0] = -INFINITY; s_n[0] = 1;
    if (LM) { s_state[0][0] = fu.m.start; s_lm[0][0] = 0.0f; }
    if (VC) { s_vstate[0][0] = 0; s_oov[0][0] = 0; }
  }
  __syncthreads();
  int cur = 0;
  for (int t = 0; t < T; t++) {
    const int nxt = cur ^ 1, n = s_n[cur];
    const float* l = logits + (row0 + t) * ld;
    const float ls = lse[row0 + t];
    const int c = topc[row0 + t].id[r];
    const float lc = topc[row0 + t].logit[r];
    // A
    if (tid < n) {
      const int last = s_last[cur][tid];
      const float tot = bm::total_of(s_pb[cur][tid], s_pnb[cur][tid]);
      s_tot[tid] = tot;
      s_spb[tid] = bm::stay_pb(tot, l[0] - ls);
      s_spnb[tid] = bm::stay_pnb(s_pnb[cur][tid], last, l[last] - ls);
    }
    if (tid == 0) s_n[nxt] = 0;
    __syncthreads();
    // B
    const bool ext = j < n && c != cc::EMPTY_ID;
    const int node = ext ? s_node[cur][j] : 0;
    float v = -INFINITY; int target = -1;
    int evstate = 0, eoov = 0;
    if (VC && ext) {   // (before the scan: see above)
      const vc::Step x = vc::step(wc.v, s_vstate[cur][j], c);
      evstate = x.next; eoov = s_oov[cur][j] + x.add;
    }
    if (ext) {
      v = bm::ext_pnb(s_pb[cur][j], s_tot[j], c == s_last[cur][j], lc - ls);
      for (int q = 0; q < n; q++)
        if (s_par[cur][q] == node && s_last[cur][q] == c) target = q;
      if (target >= 0) s_spnb[target] = bm::merged(s_spnb[target], v);
    }
    s_cand[MB + tid] = ext && target < 0 ? bm::total_of(-INFINITY, v) : -INFINITY;
    float elm = 0.0f; int estate = 0;
    if (LM || VC) {
      float key = -INFINITY;
      if (ext && target < 0) {
        const float total = s_cand[MB + tid];
        if (LM) {
          const lm::Step x = lm::step(fu.m, s_state[cur][j], c);
          elm = s_lm[cur][j] + x.score; estate = x.next;
        }
        if (VC) key = vc::key_of(total, LM ? lm::fused_of(total, elm, s_len[cur][j] + 1, fu.alpha, fu.beta) : total, eoov, wc.gamma);
        else key = lm::key_of(total, elm, s_len[cur][j] + 1, fu.alpha, fu.beta);
      }
      s_key[MB + tid] = key;
    }
    __syncthreads();
    // C
    if (tid < MB) {
      s_cand[tid] = tid < n ? bm::total_of(s_spb[tid], s_spnb[tid]) : -INFINITY;
      if (LM && !VC) s_key[tid] = tid < n ? lm::key_of(s_cand[tid], s_lm[cur][tid], s_len[cur][tid], fu.alpha, fu.beta) : -INFINITY;
      if (VC) {
        float key = -INFINITY;
        if (tid < n) {
          const float total = s_cand[tid];
          key = vc::key_of(total, LM ? lm::fused_of(total, s_lm[cur][tid], s_len[cur][tid], fu.alpha, fu.beta) : total, s_oov[cur][tid], wc.gamma);
        }
        s_key[tid] = key;
      }
    }
    __syncthreads();
    // D  (a dead candidate's key is -inf and a live one's is above it: lm::key_of)
    const float ev = rank[MB + tid], sv = tid < MB ? rank[tid] : -INFINITY;
    int eplace = bm::CANDS, splace = bm::CANDS;
    if (bm::alive(ev)) {
      eplace = 0;
      for (int k = 0; k < n; k++) eplace += cc::better(rank[k], k, ev, MB + tid) ? 1 : 0;
      for (int k = MB; k < MB + n * TC; k++) eplace += cc::better(rank[k], k, ev, MB + tid) ? 1 : 0;
    }
    if (bm::alive(sv)) {
      splace = 0;
      for (int k = 0; k < n; k++) splace += cc::better(rank[k], k, sv, tid) ? 1 : 0;
      for (int k = MB; k < MB + n * TC; k++) splace += cc::better(rank[k], k, sv, tid) ? 1 : 0;
    }
    int found = -1;
    if (eplace < B)   // (a list's head is only ever changed by an atomic in L2: read it there; tok and next are written once)
      for (int q = __hip_atomic_load(&nd[node].child, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), k = 0;
           q >= 0 && q < n_nodes && k < n_nodes && found < 0; q = nd[q].next, k++)   // (the bounds: a list never leaves the line's nodes)
        if (nd[q].tok == c) found = q;
    __syncthreads();
    // E
    if (eplace < B) {
      int id = found;
      if (id < 0) {
        id = 1 + t * B + eplace;
        const int old = atomicExch(&nd[node].child, id);
        nd[id] = bm::Node{node, c, -1, old};
      }
      s_node[nxt][eplace] = id; s_par[nxt][eplace] = node; s_last[nxt][eplace] = c; s_len[nxt][eplace] = s_len[cur][j] + 1;
      s_pb[nxt][eplace] = -INFINITY; s_pnb[nxt][eplace] = v;
      if (LM) { s_state[nxt][eplace] = estate; s_lm[nxt][eplace] = elm; }
      if (VC) { s_vstate[nxt][eplace] = evstate; s_oov[nxt][eplace] = eoov; }
      atomicMax(&s_n[nxt], eplace + 1);
    }
    if (splace < B) {
      s_node[nxt][splace] = s_node[cur][tid]; s_par[nxt][splace] = s_par[cur][tid]; s_last[nxt][splace] = s_last[cur][tid];
      s_len[nxt][splace] = s_len[cur][tid]; s_pb[nxt][splace] = s_spb[tid]; s_pnb[nxt][splace] = s_spnb[tid];
      if (LM) { s_state[nxt][splace] = s_state[cur][tid]; s_lm[nxt][splace] = s_lm[cur][tid]; }
      if (VC) { s_vstate[nxt][splace] = s_vstate[cur][tid]; s_oov[nxt][splace] = s_oov[cur][tid]; }
      atomicMax(&s_n[nxt], splace + 1);
    }
    __syncthreads();
    cur = nxt;
  }
  const int n = s_n[cur], count = n < nbest ? n : nbest;
  if (tid == 0) counts[ln.slot] = count;
  if (VC) {   // the closing phase: the final beam ranked by the closing key, then beam order (n <= B <= MB; block-uniform)
    float total = -INFINITY, fused = -INFINITY, ckey = -INFINITY; int closed = 0;
    if (tid < n) {
      total = bm::total_of(s_pb[cur][tid], s_pnb[cur][tid]);
      fused = LM ? lm::fused_of(total, s_lm[cur][tid], s_len[cur][tid], fu.alpha, fu.beta) : total;
      closed = s_oov[cur][tid] + vc::close(wc.v, s_vstate[cur][tid]);
      ckey = vc::key_of(total, fused, closed, wc.gamma);
      s_key[tid] = ckey;
    }
    __syncthreads();
    if (tid < n) {
      int place = 0;
      for (int k = 0; k < n; k++) place += cc::better(s_key[k], k, ckey, tid) ? 1 : 0;
      if (place < nbest) {
        const int len = s_len[cur][tid];
        const long long rec = (long long)ln.slot * nbest + place;
        beams[rec] = bm::Beam{total, len};
        if (LM) lms[rec] = lm::BeamLm{s_lm[cur][tid], fused};
        vocs[rec] = vc::BeamVocab{closed, vc::score_of(fused, closed, wc.gamma)};
        int* out = tokens + ln.out + (long long)place * T;
        int q = s_node[cur][tid];
        for (int i = len - 1; i >= 0 && q > 0 && q < n_nodes; i--) { out[i] = nd[q].tok; q = nd[q].parent; }
      }
    }
    return;
  }
  if (tid < count) {
    const int len = s_len[cur][tid];
    const float total = bm::total_of(s_pb[cur][tid], s_pnb[cur][tid]);
    beams[(long long)ln.slot * nbest + tid] = bm::Beam{total, len};
    if (LM) lms[(long long)ln.slot * nbest + tid] = lm::BeamLm{s_lm[cur][tid], lm::fused_of(total, s_lm[cur][tid], len, fu.alpha, fu.beta)};
    int* out = tokens + ln.out + (long long)tid * T;
    int q = s_node[cur][tid];
    for (int i = len - 1; i >= 0 && q > 0 && q < n_nodes; i--) { out[i] = nd[q].tok; q = nd[q].parent; }
  }
}
void ctc_beam_search(hipStream_t st, const float* logits, int ld, const float* lse, const bm::TopC* topc, const bm::Line* lines,
                     int n_lines, int chunk_row0, int B, int nbest, bm::Node* nodes, bm::Beam* beams, int* tokens, int* counts,
                     const lm::Fusion* fu, lm::BeamLm* lms, const vc::Constraint* wc, vc::BeamVocab* vocs) {
  if (n_lines <= 0) return;
  if (fu && wc)
    RT_LAUNCH((k_ctc_beam_search<true, true>), dim3(n_lines), dim3(256), 0, st, logits, ld, lse, topc, lines, chunk_row0, B, nbest,
              nodes, beams, tokens, counts, *fu, lms, *wc, vocs);
  else if (wc)
    RT_LAUNCH((k_ctc_beam_search<false, true>), dim3(n_lines), dim3(256), 0, st, logits, ld, lse, topc, lines, chunk_row0, B, nbest,
              nodes, beams, tokens, counts, lm::Fusion{}, nullptr, *wc, vocs);
  else if (fu)
    RT_LAUNCH((k_ctc_beam_search<true, false>), dim3(n_lines), dim3(256), 0, st, logits, ld, lse, topc, lines, chunk_row0, B, nbest,
              nodes, beams, tokens, counts, *fu, lms, vc::Constraint{}, nullptr);
  else
    RT_LAUNCH((k_ctc_beam_search<false, false>), dim3(n_lines), dim3(256), 0, st, logits, ld, lse, topc, lines, chunk_row0, B, nbest,
              nodes, beams, tokens, counts, lm::Fusion{}, nullptr, vc::Constraint{}, nullptr);
}

// Lexicon snap (ctc_lexicon_align.h).  One wave64 per lexicon line of one chunk, after k_ctc_lexicon_topk has written the line's
// matches: the wave applies the snap condition to match 0, writes snapped[slot] (0 or 1, for every line it sees) and leaves
// unless the line snaps.  Then lane s owns state s of the winner (S <= 63) and the forward pass is k_ctc_lexicon_forward's
// loop with la::best in place of lae: the same __shfl_up neighbours, the same register ring of l[t][cls(s)] loads AHEAD steps
// early, no lse, expf or logf on the chain.  A step's backpointers (0, 1 or 2 per state) leave the wave as two 64-bit ballots,
// 16 bytes per step, written by lane 0: into LDS when the line fits one tile (T <= la::TILE), otherwise into bp [2 * chunk
// rows] at the line's rows -- T has no bound beyond the pipeline's own.  The backtrack is wave-uniform and serial in t; it
// walks the line tile by tile from the end, each tile's ballots brought back coalesced (lane i loads steps i, i + 64, ...) into
// LDS first, so the chain runs over LDS reads, never over dependent global loads.  The walk leaves s_t per step in LDS, and a
// pass parallel over the tile's steps writes idx[rows[..]] = cls(s_t) and prob = expf(l - lse) through the chunk's row list.
// A backpointer cannot leave [0, S) (ctc_lexicon_align.h), so every index below stays inside the line's own rows.
// bp is deliberately NOT __restrict__: on the long-T path lane 0 writes it with plain stores and, after the __syncthreads()
// behind the forward pass (a workgroup-scope release / acquire around the barrier; the block is this one wave, on one CU and
// one L1), the other lanes read those very bytes.  Marking it __restrict__ would let the compiler treat the loads as
// independent of the stores.
__global__ __launch_bounds__(64) void k_ctc_lexicon_align(const float* __restrict__ logits, int ld, const float* __restrict__ lse,
                                                          const lx::Line* __restrict__ lines, int chunk_row0,
                                                          const lx::Lex* __restrict__ lex, const lx::Entry* __restrict__ entries,
                                                          const int* __restrict__ ids, const float* __restrict__ min_post,
                                                          const lx::Match* __restrict__ matches, const int* __restrict__ counts,
                                                          const int* __restrict__ rows, ulonglong2* bp, int* __restrict__ idx,
                                                          float* __restrict__ prob, int* __restrict__ snapped,
                                                          float* __restrict__ vit) {
  constexpr int AHEAD = 4, TILE = la::TILE;
  __shared__ ulonglong2 s_bp[TILE];
  __shared__ unsigned char s_state[TILE];
  const int lane = threadIdx.x;
  const lx::Line ln = lines[blockIdx.x];
  const float mp = min_post[ln.lex];
  bool fire = false; int e = 0;
  if (mp > 0.0f) {   // (a match slot past the count was never written: read match 0 only where there is one)
    const int cnt = counts[ln.slot];
    if (cnt >= 1) {
      const lx::Match m = matches[(long long)ln.slot * lx::MATCHES];
      fire = la::snaps(mp, cnt, m.posterior); e = m.entry;
    }
  }
  if (lane == 0) snapped[ln.slot] = fire ? 1 : 0;
  if (!fire) return;   // (wave-uniform)
  const lx::Entry E = entries[lex[ln.lex].first + e];
  const int32_t* eid = ids + E.off;
  const int s = lane, S = 2 * E.len + 1, T = ln.T;
  const bool mine = s < S;
  const int cls = mine ? lx::cls_of(eid, s) : 0;
  const bool skip = mine && lx::skip_of(eid, s);
  const long long r0 = ln.row0 - chunk_row0;
  const float* col = logits + r0 * ld + cls;
  const bool in_lds = T <= TILE;
  ulonglong2* g = bp + r0;
  float lq[AHEAD];
#pragma unroll
  for (int j = 0; j < AHEAD; j++) lq[j] = j < T ? col[(long long)j * ld] : 0.0f;
  float v = -INFINITY;
  for (int t0 = 0; t0 < T; t0 += AHEAD) {
#pragma unroll
    for (int j = 0; j < AHEAD; j++) {
      const int t = t0 + j;
      if (t < T) {   // (wave-uniform)
        const float l = lq[j];
        if (t + AHEAD < T) lq[j] = col[(long long)(t + AHEAD) * ld];
        const float u1 = __shfl_up(v, 1), u2 = __shfl_up(v, 2);
        int off;
        const float b = la::best(v, s >= 1 ? u1 : -INFINITY, skip ? u2 : -INFINITY, &off);
        const float nx = t == 0 ? (s < 2 ? l : -INFINITY) : b + l;
        v = mine ? nx : -INFINITY;
        if (t == 0 || !mine) off = 0;
        const ulonglong2 q = make_ulonglong2(__ballot(off & 1), __ballot(off >> 1));
        if (lane == 0) { if (in_lds) s_bp[t] = q; else g[t] = q; }
      }
    }
  }
  const float f1 = __shfl(v, S - 1), f2 = __shfl(v, S - 2);
  int cur = __builtin_amdgcn_readfirstlane(la::end_of(f1, f2, S));
  if (lane == 0 && vit) vit[ln.slot] = cur == S - 1 ? f1 : f2;
  __syncthreads();   // (lane 0's ballots, in LDS or in bp, before any lane reads them)
  for (int t1 = T; t1 > 0;) {
    const int tb = in_lds ? 0 : ((t1 - 1) / TILE) * TILE, n = t1 - tb;   // the tile [tb, t1), n <= TILE
    if (!in_lds) {
      for (int i = lane; i < n; i += 64) s_bp[i] = g[tb + i];
      __syncthreads();
    }
    for (int i = n - 1; i >= 0; i--) {
      const ulonglong2 q = s_bp[i];
      if (lane == 0) s_state[i] = (unsigned char)cur;
      cur -= __builtin_amdgcn_readfirstlane((int)((q.x >> cur) & 1ull) | ((int)((q.y >> cur) & 1ull) << 1));
    }
    __syncthreads();
    for (int i = lane; i < n; i += 64) {
      const int c = lx::cls_of(eid, s_state[i]), row = rows[ln.row0 + tb + i];
      idx[row] = c;
      prob[row] = expf(logits[(r0 + tb + i) * ld + c] - lse[r0 + tb + i]);
    }
    __syncthreads();   // (the tile's states and ballots are read before the next tile overwrites them)
    t1 = tb;
  }
}
void ctc_lexicon_align(hipStream_t st, const float* logits, int ld, const float* lse, const lx::Line* lines, int n_lines,
                       int chunk_row0, const lx::Lex* lex, const lx::Entry* entries, const int* ids, const float* min_post,
                       const lx::Match* matches, const int* counts, const int* rows, void* bp, int* idx, float* prob, int* snapped,
                       float* vit) {
  if (n_lines <= 0) return;
  RT_LAUNCH(k_ctc_lexicon_align, dim3(n_lines), dim3(64), 0, st, logits, ld, lse, lines, chunk_row0, lex, entries, ids, min_post,
            matches, counts, rows, static_cast<ulonglong2*>(bp), idx, prob, snapped, vit);
}

// Rec patterns (ctc_pattern.h).  One wave64 per row i < m of logits [m][ld]: rmax[i] = the largest logit of the columns <
// classes, k_ctc_row_lse's first pass (free_logprob needs it beside the lse; that kernel and its result stay as they are).
__global__ __launch_bounds__(64) void k_ctc_row_max(const float* __restrict__ logits, int ld, int classes, int m,
                                                    float* __restrict__ rmax) {
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= m) return;
  const float4* x = reinterpret_cast<const float4*>(logits + (long long)i * ld);
  const int nv = (classes + 3) / 4;
  float mx = -INFINITY;
  for (int v = lane; v < nv; v += 64) {
    const float4 q = x[v];
    const float e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (4 * v + u < classes && e[u] > mx) mx = e[u];   // (pt::viterbi_line's comparison: a NaN never becomes the maximum)
  }
  for (int o = 32; o >= 1; o >>= 1) { const float w = __shfl_xor(mx, o); if (w > mx) mx = w; }
  if (lane == 0) rmax[i] = mx;
}
void ctc_row_max(hipStream_t st, const float* logits, int ld, int classes, int m, float* rmax) {
  if (m <= 0) return;
  RT_LAUNCH(k_ctc_row_max, dim3(m), dim3(64), 0, st, logits, ld, classes, m, rmax);
}

// The pattern Viterbi of ctc_pattern.h.  One workgroup of 256 threads per pattern line of one chunk.  B and C of two steps live
// in LDS (2 x (64 + 4096) floats at the caps), beside the pattern's pair classes (16 bits each), its seg table and -- when they
// are at most PREDS_LDS bytes -- its predecessor lists.  A step has three parts between two barriers:
//   1. top(q): wave w takes the states q = w, w + 4, ...; its lanes stride over the state's pairs, each keeping a pt::Top of
//      the live values it saw, and an xor butterfly merges the 64 lists with pt::top_insert (the lists of the two halves are
//      disjoint at every level, and the order (value, pair index) is total over live values, so the result is the serial scan's);
//   2. thread i updates the pairs i, i + 256, ... over their predecessor lists (pt::into_of) and stores one 16-bit code each;
//   3. lane q of wave 0 updates B[q].
// l[t][c] of a thread's pairs and of the blank is loaded one step ahead into registers, right behind its use: the gather is
// off the chain.  The codes of step t go to row t of the line's table, P + S codes wide: in LDS when T * (P + S) <= pt::BP_LDS,
// otherwise at bp + line.bp in the chunk's scratch buffer; the same generic pointer serves both.  After the last step thread 0
// picks the end node and walks the table back, serial in t, leaving each step's node in slot 0 of its row (a row's code is
// read before its slot 0 is overwritten; row 0 holds no codes); meanwhile thread 64 adds up lse and rmax in t order.  The rows
// are then written back in parallel.  No code outside [0, S) / [0, P) is ever stored or followed (ctc_pattern.h).
// bp is not __restrict__: other threads read what a thread stored, across the barriers.
constexpr int PREDS_LDS = 2048;   // a pattern's predecessor bytes (one per arc) that the kernel copies into LDS
__global__ __launch_bounds__(256) void k_ctc_pattern_viterbi(const float* __restrict__ logits, int ld, const float* __restrict__ lse,
                                                             const float* __restrict__ rmax, const pt::Line* __restrict__ lines,
                                                             int chunk_row0, pt::DevTables tb, const int* __restrict__ rows,
                                                             uint16_t* bp_mem, int* __restrict__ idx, float* __restrict__ prob,
                                                             int* __restrict__ matched, float* __restrict__ vit,
                                                             float* __restrict__ logprob, float* __restrict__ free_lp) {
  constexpr int NT = 256, PER = pt::MAX_PAIRS / NT;
  __shared__ float sB[2][pt::MAX_STATES];
  __shared__ float sC[2][pt::MAX_PAIRS];
  __shared__ float sV1[pt::MAX_STATES], sV2[pt::MAX_STATES];
  __shared__ int sA1[pt::MAX_STATES], sA2[pt::MAX_STATES], sK1[pt::MAX_STATES], sSeg[pt::MAX_STATES + 1];
  __shared__ uint16_t sPC[pt::MAX_PAIRS];
  __shared__ uint16_t sBP[pt::BP_LDS];
  __shared__ uint8_t sPreds[PREDS_LDS];
  __shared__ float sSum[2];
  __shared__ int sEnd;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const pt::Line ln = lines[blockIdx.x];
  const pt::Pat pat = tb.pats[ln.pat];
  const int S = pat.S, P = pat.P, T = ln.T, W = P + S;
  if (T < 1) {   // (uniform)
    if (tid == 0) { matched[ln.slot] = 0; vit[ln.slot] = -INFINITY; logprob[ln.slot] = -INFINITY; free_lp[ln.slot] = 0.0f; }
    return;
  }
  const long long r0 = ln.row0 - chunk_row0;
  const float* L = logits + r0 * ld;
  uint16_t* bp = pt::bp_codes(T, P, S) <= pt::BP_LDS ? sBP : bp_mem + ln.bp;
  const bool preds_in_lds = pat.n_pred <= PREDS_LDS;
  const uint8_t* pr = preds_in_lds ? sPreds : tb.preds + pat.pred0;
  for (int p = tid; p < P; p += NT) sPC[p] = (uint16_t)tb.pair_c[pat.pair0 + p];
  for (int q = tid; q <= S; q += NT) sSeg[q] = tb.seg[pat.seg0 + q];
  if (preds_in_lds) for (int j = tid; j < pat.n_pred; j += NT) sPreds[j] = tb.preds[pat.pred0 + j];
  int pb[PER], pe[PER];
  float lq[PER];
#pragma unroll
  for (int k = 0; k < PER; k++) {
    const int p = tid + k * NT;
    pb[k] = p < P ? tb.pair_pb[pat.pair0 + p] : 0; pe[k] = p < P ? tb.pair_pe[pat.pair0 + p] : 0;
  }
  __syncthreads();
  // t = 0
  if (tid < S) sB[0][tid] = tid == 0 ? L[0] : -INFINITY;
  float lb = tid < S && T > 1 ? L[ld] : 0.0f;
#pragma unroll
  for (int k = 0; k < PER; k++) {
    const int p = tid + k * NT;
    lq[k] = 0.0f;
    if (p < P) {
      const int c = sPC[p];
      sC[0][p] = pr[pb[k]] == 0 ? L[c] : -INFINITY;
      if (T > 1) lq[k] = L[ld + c];
    }
  }
  __syncthreads();
  int cur = 0;
  for (int t = 1; t <= T; t++) {   // (t == T: top() of the last step alone, for the end)
    for (int q = wave; q < S; q += NT / 64) {
      pt::Top tp = pt::top_empty();
      for (int p = sSeg[q] + lane; p < sSeg[q + 1]; p += 64) { const float v = sC[cur][p]; if (v > -INFINITY) pt::top_insert(tp, v, p); }
      for (int o = 32; o >= 1; o >>= 1) {
        const float w1 = __shfl_xor(tp.v1, o), w2 = __shfl_xor(tp.v2, o);
        const int b1 = __shfl_xor(tp.a1, o), b2 = __shfl_xor(tp.a2, o);
        pt::top_insert(tp, w1, b1); pt::top_insert(tp, w2, b2);   // (an empty slot, (-inf, NONE), ranks before nothing)
      }
      if (lane == 0) { sV1[q] = tp.v1; sV2[q] = tp.v2; sA1[q] = tp.a1; sA2[q] = tp.a2; sK1[q] = tp.a1 == pt::NONE ? 0 : sPC[tp.a1]; }
    }
    __syncthreads();
    if (t == T) break;
    const int nxt = cur ^ 1;
    uint16_t* row = bp + (long long)t * W;
    const float* Ln = L + (long long)(t + 1) * ld;
    const bool more = t + 1 < T;
#pragma unroll
    for (int k = 0; k < PER; k++) {
      const int p = tid + k * NT;
      if (p < P) {
        const int c = sPC[p];
        float best = sC[cur][p]; int code = pt::STAY;
        for (int j = pb[k]; j < pe[k]; j++) {
          const int q = pr[j];
          int kc;
          const float v = pt::into_of(sB[cur][q], q, pt::Top{sV1[q], sV2[q], sA1[q], sA2[q]}, sK1[q], c, &kc);
          if (v > best) { best = v; code = kc; }
        }
        sC[nxt][p] = lq[k] + best;
        row[p] = (uint16_t)code;
        if (more) lq[k] = Ln[c];
      }
    }
    if (tid < S) {
      float best = sB[cur][tid]; int code = pt::STAY;
      if (sV1[tid] > best) { best = sV1[tid]; code = sA1[tid]; }
      sB[nxt][tid] = lb + best;
      row[P + tid] = (uint16_t)code;
      if (more) lb = Ln[0];
    }
    __syncthreads();
    cur = nxt;
  }
  if (tid == 0) {
    float best = -INFINITY; int node = pt::NONE;
    for (int q = 0; q < S; q++) {
      if (!((pat.accept >> q) & 1ull)) continue;
      if (sB[cur][q] > best) { best = sB[cur][q]; node = pt::BLANK | q; }
      if (sV1[q] > best) { best = sV1[q]; node = sA1[q]; }
    }
    sEnd = node;
    sSum[0] = best;
    if (node != pt::NONE) {
      for (int t = T - 1; t >= 0; t--) {
        const int here = node;
        if (t > 0) {
          const int k = bp[(long long)t * W + ((node & pt::BLANK) ? P + (node & ~pt::BLANK) : node)];
          if (k != pt::STAY) node = k;
        }
        bp[(long long)t * W] = (uint16_t)here;
      }
    }
  }
  float sum_lse = 0.0f, fr = 0.0f;
  if (tid == 64) {
    for (int t = 0; t < T; t++) { fr = fr + (rmax[r0 + t] - lse[r0 + t]); sum_lse = sum_lse + lse[r0 + t]; }
    sSum[1] = fr;
  }
  __syncthreads();
  const bool hit = sEnd != pt::NONE;
  if (tid == 64) {
    matched[ln.slot] = hit ? 1 : 0; vit[ln.slot] = hit ? sSum[0] : -INFINITY; logprob[ln.slot] = hit ? sSum[0] - sum_lse : -INFINITY;
    free_lp[ln.slot] = fr;
  }
  if (!hit) return;
  for (int t = tid; t < T; t += NT) {
    const int node = bp[(long long)t * W];
    const int c = (node & pt::BLANK) ? 0 : sPC[node], r = rows[ln.row0 + t];
    idx[r] = c;
    prob[r] = expf(L[(long long)t * ld + c] - lse[r0 + t]);
  }
}
void ctc_pattern_viterbi(hipStream_t st, const float* logits, int ld, int classes, const float* lse, const float* rmax,
                         const pt::Line* lines, int n_lines, int chunk_row0, const pt::DevTables& tb, const int* rows, void* bp,
                         int* idx, float* prob, int* matched, float* vit, float* logprob, float* free_lp) {
  if (n_lines <= 0) return;
  if (classes > 65535) throw RtError(4, "ctc_pattern_viterbi: more than 65535 classes");   // (pair classes are 16 bits in LDS)
  RT_LAUNCH(k_ctc_pattern_viterbi, dim3(n_lines), dim3(256), 0, st, logits, ld, lse, rmax, lines, chunk_row0, tb, rows,
            static_cast<uint16_t*>(bp), idx, prob, matched, vit, logprob, free_lp);
}

// ===========================================================================
// (round 5: 8192 values per block, 16-byte loads -- was 65536 per block, scalar: one 960 x 960 map ran on 15 workgroups for 77 us,
//  6 % of the C2 call)
constexpr int SUM_PER_BLOCK = 8192;
int sum_blocks(long long n) { return (int)((n + SUM_PER_BLOCK - 1) / SUM_PER_BLOCK); }
__global__ __launch_bounds__(256) void k_sum_partial(const float* __restrict__ x, long long n, double* __restrict__ partials) {
  __shared__ double red[256];
  const long long base = (long long)blockIdx.x * SUM_PER_BLOCK;
  double s = 0.0;
  if ((((size_t)x & 15) == 0) && base + SUM_PER_BLOCK <= n) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x + base);
#pragma unroll
    for (int i = 0; i < SUM_PER_BLOCK / 1024; i++) { const f32x4 v = x4[threadIdx.x + 256 * i]; s += (double)v[0] + (double)v[1] + (double)v[2] + (double)v[3]; }
  } else {
    for (int i = threadIdx.x; i < SUM_PER_BLOCK; i += 256) { long long k = base + i; if (k < n) s += (double)x[k]; }
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
  if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}
void sum_partial(hipStream_t st, const float* x, long long n, double* partials) {
  if (n <= 0) return;
  RT_LAUNCH(k_sum_partial, dim3(sum_blocks(n)), dim3(256), 0, st, x, n, partials);
}

// ---- det tiles (det_tiles.h): pure data movement, one launch per det group each, blockIdx.y = tile of the group -------------
// Both walk a tile in 16-byte vectors, rows coalesced, with a grid-stride loop over at most DT_MAX_BLOCKS_X blocks a tile (a
// 960 x 960 tile is 172 800 vectors to cut, up to 230 400 to stitch).  Everything is inside its buffers by the plan: a tile lies
// inside its page, an owned rectangle inside its tile.
#define DT_MAX_BLOCKS_X 256
// cut: the tile's th rows of tw * 3 bytes -> contiguous at cut + cut_off.  tw, x0 and page_w are multiples of 32, so a row is
// tw * 3 / 16 whole vectors and starts a multiple of 96 bytes from the page's first byte: with the page 16-byte aligned (every
// page the session made itself; a caller's device page that was not resized need not be) loads and stores are 16 bytes wide,
// otherwise the loads are bytes.
__global__ __launch_bounds__(256) void k_det_tile_cut(const dt::TileDesc* __restrict__ tiles, u8* __restrict__ cut) {
  const dt::TileDesc d = tiles[blockIdx.y];
  const int vpr = d.tw * 3 / 16;
  const long long total = (long long)d.th * vpr;
  u8* dst = cut + d.cut_off;
  const bool al = ((size_t)d.src & 15) == 0;
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < total; v += (long long)gridDim.x * 256) {
    const int r = (int)(v / vpr), c = (int)(v - (long long)r * vpr);
    const u8* s = d.src + ((long long)(d.y0 + r) * d.page_w + d.x0) * 3 + (long long)c * 16;
    uint4 w;
    if (al) w = *reinterpret_cast<const uint4*>(s);
    else {
      unsigned q[4];
#pragma unroll
      for (int k = 0; k < 4; k++) q[k] = (unsigned)s[4 * k] | ((unsigned)s[4 * k + 1] << 8) | ((unsigned)s[4 * k + 2] << 16) | ((unsigned)s[4 * k + 3] << 24);
      w = make_uint4(q[0], q[1], q[2], q[3]);
    }
    *reinterpret_cast<uint4*>(dst + v * 16) = w;
  }
}
void det_tile_cut(hipStream_t st, const dt::TileDesc* tiles, int n, long long max_tile_pix, uint8_t* cut) {
  if (n <= 0 || max_tile_pix <= 0) return;
  const long long want = (max_tile_pix * 3 / 16 + 255) / 256;
  RT_LAUNCH(k_det_tile_cut, dim3((unsigned)std::min<long long>(want, DT_MAX_BLOCKS_X), n), dim3(256), 0, st, tiles, cut);
}
// stitch: the tile's owned rectangle, (ox1 - ox0) / 4 float4 a row (ownership bounds are multiples of 16), from its map into the
// page map.  The owned rectangles of a page's tiles partition the page: every page pixel is written once over the call, plain stores.
__global__ __launch_bounds__(256) void k_det_tile_stitch(const dt::TileDesc* __restrict__ tiles, const float* __restrict__ maps) {
  const dt::TileDesc d = tiles[blockIdx.y];
  const int vpr = (d.ox1 - d.ox0) / 4;
  const long long total = (long long)(d.oy1 - d.oy0) * vpr;
  const float* src = maps + d.map_off;
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < total; v += (long long)gridDim.x * 256) {
    const int r = (int)(v / vpr), c = (int)(v - (long long)r * vpr);
    const float4 w = *reinterpret_cast<const float4*>(src + (long long)(d.oy0 - d.y0 + r) * d.tw + (d.ox0 - d.x0) + 4 * c);
    *reinterpret_cast<float4*>(d.page_map + (long long)(d.oy0 + r) * d.page_w + d.ox0 + 4 * c) = w;
  }
}
void det_tile_stitch(hipStream_t st, const dt::TileDesc* tiles, int n, long long max_tile_pix, const float* maps) {
  if (n <= 0 || max_tile_pix <= 0) return;
  const long long want = (max_tile_pix / 4 + 255) / 256;
  RT_LAUNCH(k_det_tile_stitch, dim3((unsigned)std::min<long long>(want, DT_MAX_BLOCKS_X), n), dim3(256), 0, st, tiles, maps);
}

// ---- rec windows (rec_windows.h): pure data movement, one launch per windowed rec group each, blockIdx.y = unit of the group --
// Both walk a unit in 16-byte vectors with a grid-stride loop over at most RW_MAX_BLOCKS_X blocks a unit (a 48 x 640 unit is
// 30 720 vectors to cut; a unit that owns 64 steps is 2048 lanes to stitch).  Everything is inside its buffers by the plan: a
// unit's columns lie inside its line, its owned steps inside its own rows and inside the line's.
#define RW_MAX_BLOCKS_X 64
// cut: the unit's h rows of w pixels (one float4 each: NHWC-4) out of the line's rows of line_w pixels -> contiguous at unit +
// dst_off.  Consecutive threads read and write consecutive pixels of a row.
__global__ __launch_bounds__(256) void k_rec_window_cut(const rw::UnitDesc* __restrict__ units, int h, const float4* __restrict__ lines,
                                                        float4* __restrict__ unit) {
  const rw::UnitDesc d = units[blockIdx.y];
  const long long total = (long long)h * d.w;
  const float4* src = lines + d.src_off + d.x0;
  float4* dst = unit + d.dst_off;
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < total; v += (long long)gridDim.x * 256) {
    const int r = (int)(v / d.w), c = (int)(v - (long long)r * d.w);
    dst[v] = src[(long long)r * d.line_w + c];
  }
}
void rec_window_cut(hipStream_t st, const rw::UnitDesc* units, int n, int h, int max_w, const float* lines, float* unit) {
  if (n <= 0 || h <= 0 || max_w <= 0) return;
  const long long want = ((long long)h * max_w + 255) / 256;
  RT_LAUNCH(k_rec_window_cut, dim3((unsigned)std::min<long long>(want, RW_MAX_BLOCKS_X), n), dim3(256), 0, st, units, h,
            reinterpret_cast<const float4*>(lines), reinterpret_cast<float4*>(unit));
}
// stitch: 32 lanes a row -- lanes 0..29 the row's 30 float4 of z5 (skipped without z5), lane 30 its idx, lane 31 its prob -- from
// the unit's row t - m into the line's row t, for the steps [t0, t1) the unit owns.  The owned steps of a line's units partition
// its rows: every line row is written once over the launch, plain stores.
__global__ __launch_bounds__(256) void k_rec_window_stitch(const rw::UnitDesc* __restrict__ units, const int* __restrict__ unit_idx,
                                                           const float* __restrict__ unit_prob, const float4* __restrict__ unit_z5,
                                                           int* __restrict__ line_idx, float* __restrict__ line_prob,
                                                           float4* __restrict__ line_z5) {
  const rw::UnitDesc d = units[blockIdx.y];
  const long long total = (long long)(d.t1 - d.t0) * 32;
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < total; v += (long long)gridDim.x * 256) {
    const int t = d.t0 + (int)(v >> 5), lane = (int)(v & 31);
    const long long s = d.unit_row + (t - d.m), o = d.line_row + t;
    if (lane < rw::Z5_D / 4) { if (unit_z5) line_z5[o * (rw::Z5_D / 4) + lane] = unit_z5[s * (rw::Z5_D / 4) + lane]; }
    else if (lane == 30) line_idx[o] = unit_idx[s];
    else line_prob[o] = unit_prob[s];
  }
}
void rec_window_stitch(hipStream_t st, const rw::UnitDesc* units, int n, int max_rows, const int* unit_idx, const float* unit_prob,
                       const float* unit_z5, int* line_idx, float* line_prob, float* line_z5) {
  if (n <= 0 || max_rows <= 0) return;
  static_assert(rw::Z5_D / 4 == 30, "k_rec_window_stitch gives a z5 row 30 of its 32 lanes");
  const long long want = ((long long)max_rows * 32 + 255) / 256;
  RT_LAUNCH(k_rec_window_stitch, dim3((unsigned)std::min<long long>(want, RW_MAX_BLOCKS_X), n), dim3(256), 0, st, units, unit_idx,
            unit_prob, reinterpret_cast<const float4*>(unit_z5), line_idx, line_prob, reinterpret_cast<float4*>(line_z5));
}

// ---- rec flip (rec_flip.h): pure data movement --------------------------------------------------------------------------
// rotate: the flagged crops of a rec group as one flat list of pixels, the way k_warp_crops_flat walks its crops (their sizes
// differ by orders of magnitude).  Thread g writes destination pixel p = g - pix_base of its crop from source pixel npix - 1 - p:
// a byte permutation in whole pixels.  Consecutive threads write consecutive pixels and read consecutive pixels backwards, so a
// wave's 192 bytes lie in the same cache lines either way.  Inside its buffers by the table: p < npix on both sides.
__global__ __launch_bounds__(256) void k_rec_flip_rotate(const rf::FlipCrop* __restrict__ crops, int n, long long total,
                                                         const u8* __restrict__ pool, u8* __restrict__ flipped) {
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long long)gridDim.x * 256) {
    const rf::FlipCrop& c = crops[rf::find_crop(crops, n, g)];
    const long long p = g - c.pix_base;
    if (p < 0 || p >= c.npix) continue;   // (a table whose bases do not match its sizes writes nothing)
    const u8* a = pool + c.src_off + rf::src_pixel(c.npix, p) * 3;
    u8* q = flipped + c.dst_off + p * 3;
    const u8 r = a[0], gg = a[1], b = a[2];
    q[0] = r; q[1] = gg; q[2] = b;
  }
}
void rec_flip_rotate(hipStream_t st, const rf::FlipCrop* crops, int n, long long total_pix, const uint8_t* pool, uint8_t* flipped) {
  if (n <= 0 || total_pix <= 0) return;
  const long long want = (total_pix + 255) / 256;
  RT_LAUNCH(k_rec_flip_rotate, dim3((unsigned)std::min<long long>(want, WARP_FLAT_MAX_BLOCKS)), dim3(256), 0, st, crops, n, total_pix,
            pool, flipped);
}
// select: blockIdx.y = both-ways line of the group.  Every thread reads the two views' (kept tokens, score) -- k_ctc_decode's
// outputs over the views -- and applies rf::choose; the block's first thread writes the outcome and the two scores.  Then the
// chosen view's T rows go to the line's rows, 32 lanes a row as k_rec_window_stitch: lanes 0..29 the row's 30 float4 of z5,
// lane 30 its idx, lane 31 its prob.  z5 and v_z5 are ONE buffer (the lines' rows are the views' prefix, rec_flip.h): a kept
// view 0 is in place and only a taken view 1 is moved, from rows behind the prefix, so no thread reads what another writes.
__global__ __launch_bounds__(256) void k_rec_flip_select(const rf::SelectDesc* __restrict__ lines, const int* __restrict__ v_ntok,
                                                         const float* __restrict__ v_score, const int* __restrict__ v_idx,
                                                         const float* __restrict__ v_prob, const float4* v_z5, int* __restrict__ idx,
                                                         float* __restrict__ prob, float4* z5, int* __restrict__ outcome,
                                                         float* __restrict__ scores) {
  const rf::SelectDesc d = lines[blockIdx.y];
  const float s0 = v_score[d.v0], s1 = v_score[d.v1];
  const int take = rf::choose(v_ntok[d.v0], s0, v_ntok[d.v1], s1);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    outcome[d.slot] = take ? rf::TOOK_1 : rf::KEPT_0;
    scores[2 * (long long)d.slot] = s0; scores[2 * (long long)d.slot + 1] = s1;
  }
  const long long src = take ? d.row1 : d.row0;
  const long long total = (long long)d.T * 32;
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < total; v += (long long)gridDim.x * 256) {
    const int t = (int)(v >> 5), lane = (int)(v & 31);
    const long long s = src + t, o = d.out_row + t;
    if (lane < rw::Z5_D / 4) { if (v_z5 && take) z5[o * (rw::Z5_D / 4) + lane] = v_z5[s * (rw::Z5_D / 4) + lane]; }
    else if (lane == 30) idx[o] = v_idx[s];
    else prob[o] = v_prob[s];
  }
}
void rec_flip_select(hipStream_t st, const rf::SelectDesc* lines, int n, int max_T, const int* v_ntok, const float* v_score,
                     const int* v_idx, const float* v_prob, float* v_z5, int* idx, float* prob, int* outcome, float* scores) {
  if (n <= 0) return;
  static_assert(rw::Z5_D / 4 == 30, "k_rec_flip_select gives a z5 row 30 of its 32 lanes");
  const long long want = std::max<long long>(((long long)max_T * 32 + 255) / 256, 1);   // (T = 0: the outcome is still written)
  RT_LAUNCH(k_rec_flip_select, dim3((unsigned)std::min<long long>(want, RW_MAX_BLOCKS_X), n), dim3(256), 0, st, lines, v_ntok, v_score,
            v_idx, v_prob, reinterpret_cast<const float4*>(v_z5), idx, prob, reinterpret_cast<float4*>(v_z5), outcome, scores);
}

}  // namespace pp
}  // namespace rt
