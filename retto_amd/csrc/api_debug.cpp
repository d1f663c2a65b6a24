// Kernel-level diagnostics of libretto_hip.so (include/retto_hip.h, diagnostics section): the A/B switches of tools/, the kernel
// micro-benchmarks (rt_bench_*), and one harness per kernel family that runs a single launch on host arrays for the fp64 tests
// (rt_debug_gemm, _dwconv, _dw_plan, _attention, _lc_block, _lc_wide, _conv13, _layernorm, _conv16, _glue16, _fpn, _conv16x, _cls_block, _stem, _glue32).
// None of it runs in production, and every kernel test depends on it.  A harness has one shape: check the arguments (each
// failure with its own message, before any device work), lay the ragged lists out (Ragged, api_internal.h), put the operands on the device
// (DevBufs::upload / zeroed, upload_as), fill what the kernel writes with RT_DEBUG_CANARY and spare rows (DevBufs::canary),
// launch as the networks do, synchronise the stream, DevBufs::download.  A new entry is a thin body on these helpers.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "api_internal.h"

using namespace rt;

namespace {
using nh::half_t;

// fp16 conv weights [cout][cin][kh][kw] as upload_conv16 packs them: [ceil(cin_pad / 32)][kh][kw][npad][32] halves, zero where
// no weight lands.  rt_debug_conv16 passes cin_pad = pitch8(cin), rt_debug_conv16x cin_pad = cin (a multiple of 8 there); the
// slab count is ceil(cin / 32) either way: ceil(cin / 32) * 32 is a multiple of 8 that is >= cin, hence >= pitch8(cin), so
// ceil(pitch8(cin) / 32) <= ceil(cin / 32), and pitch8(cin) >= cin gives the other direction.  The buffers are the same bytes.
std::vector<half_t> pack_conv16_weights(const float* wt, int cout, int cin, int kh, int kw, int cin_pad) {
  const int npad = round_up(cout, 32), nslab = (cin_pad + nh::KS - 1) / nh::KS;
  std::vector<half_t> hw((size_t)nslab * kh * kw * npad * nh::KS, (half_t)0.f);
  for (int n = 0; n < cout; n++)
    for (int k = 0; k < cin; k++)
      for (int t = 0; t < kh * kw; t++)
        hw[(((size_t)(k / nh::KS) * kh * kw + t) * npad + n) * nh::KS + k % nh::KS] = (half_t)wt[((size_t)n * cin + k) * kh * kw + t];
  return hw;
}

// the step the GEMM benchmarks' operand generators share (each maps the state to its own distribution)
inline uint64_t xorshift64(uint64_t& s) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }

// The tail of a kernel micro-benchmark: one warm launch, `iters` timed ones (*ms_out = the mean), then max |d0 - d1| over the
// first and the last min(total, 4 M) elements (the last row block is the partial one); a NaN difference counts as infinity.
template <typename F>
void timed_and_compared(hipStream_t st, int iters, F&& launch, const float* d0, const float* d1, size_t total, float* ms_out, float* maxdiff_out) {
  launch();
  Events ev; RT_HIP_CHECK(hipEventCreate(&ev.a)); RT_HIP_CHECK(hipEventCreate(&ev.b));
  RT_HIP_CHECK(hipEventRecord(ev.a, st));
  for (int i = 0; i < iters; i++) launch();
  RT_HIP_CHECK(hipEventRecord(ev.b, st));
  RT_HIP_CHECK(hipStreamSynchronize(st));
  float ms = 0; RT_HIP_CHECK(hipEventElapsedTime(&ms, ev.a, ev.b)); *ms_out = ms / iters;
  if (!maxdiff_out) return;
  const size_t cnt = std::min<size_t>(total, (size_t)1 << 22);
  std::vector<float> c0(cnt), c1(cnt);
  float md = 0;
  for (size_t off : {(size_t)0, total - cnt}) {
    DevBufs::download(c0.data(), d0 + off, cnt); DevBufs::download(c1.data(), d1 + off, cnt);
    for (size_t i = 0; i < cnt; i++) { const float d = std::fabs(c0[i] - c1[i]); md = (d > md || d != d) ? (d != d ? INFINITY : d) : md; }
  }
  *maxdiff_out = md;
}

// A/B switches for tools/ (include/retto_hip.h, diagnostics section)
// what the environment selected when the library was loaded (dynamic initialisation runs after the nn:: globals of the other
// translation units only by luck of link order, so these are read on the first call of rt_create -- before any hook can have
// changed them -- see capture_variant_defaults())
int g_default_lc_wave = 3, g_default_gemm_dma = 1, g_default_dw_sweep = 4, g_default_cls_fused = 1, g_default_gemm_split = 0;
}  // namespace

void rt::capture_variant_defaults() {
  static const bool once = [] {
    g_default_lc_wave = nn::g_lc_wave; g_default_gemm_dma = nn::g_gemm_dma; g_default_dw_sweep = nn::g_dw_sweep; g_default_cls_fused = nn::g_cls_fused; g_default_gemm_split = nn::g_gemm_split;
    return true;
  }();
  (void)once;
}

extern "C" {

RT_API void rt_debug_set_variants(int gemm_variant, int dw_variant, int flags) {
  capture_variant_defaults();
  (void)dw_variant;   // (no effect; bits 1-5 of flags neither)
  nn::g_gemm_variant = gemm_variant;
  nn::g_argmax_wide = (flags & 64) ? 2 : 0;
  // round-3 kernels: bits 7-9 send their layers back to the kernels they replaced (defaults = what the environment selected at load)
  const int lc_wave0 = g_default_lc_wave, gemm_dma0 = g_default_gemm_dma, dw_sweep0 = g_default_dw_sweep, cls_fused0 = g_default_cls_fused;
  nn::g_lc_wave = (flags & 128) ? 0 : lc_wave0;
  nn::g_gemm_dma = (flags & 256) ? 0 : gemm_dma0;
  nn::g_dw_sweep = (flags & 512) ? 0 : dw_sweep0;
  nn::g_fpn_phase_off = (flags & 2048) ? 1 : 0;   // (bit 11: RSEFPN / DB-head convs as the round-3 launch series; not bit-identical: both forms stand against fp64 in tests/test_gpu_fpn_kernels.py)
  nn::g_gemm_split = (flags & 4096) ? 1 : g_default_gemm_split;   // (bit 12: the split-bf16 form of the wide rec-net GEMMs, opt-in)
  nn::g_cls_fused = (flags & 1024) ? 0 : cls_fused0;   // (bit 10: the classifier's blocks as the unfused launch series; fp32-tolerance equal, not bit-identical)
}
// Runs one nh::conv16 launch on host tensors (diagnostics: the numerics tests compare it with torch conv2d).
// x [n, cin, h, w] f32, w [cout, cin, kh, kw] f32, bias [cout] or null, "same" padding k/2, stride (sh, sw); out [n, cout, ho, wo] f32.
RT_API int rt_debug_conv16(rt_session* s, const float* x, int n, int cin, int h, int w, const float* wt, int cout, int kh, int kw,
                           int sh, int sw, const float* bias, int act, float* out) {
  RT_REQUIRE(s && x && wt && out && n > 0 && cin > 0 && h > 0 && w > 0 && cout > 0, s, "rt_debug_conv16: bad argument");
  return guarded(s, [&] {
    s->begin_call();
    const int cp = nh::pitch8(cin), op = nh::pitch8(cout), npad = round_up(cout, 32);
    const int ho = (h - 1) / sh + 1, wo = (w - 1) / sw + 1;
    std::vector<half_t> hx((size_t)n * h * w * cp, (half_t)0.f);
    const std::vector<half_t> hw = pack_conv16_weights(wt, cout, cin, kh, kw, cp);
    for (int i = 0; i < n; i++)
      for (int c = 0; c < cin; c++)
        for (int p = 0; p < h * w; p++) hx[((size_t)i * h * w + p) * cp + c] = (half_t)x[((size_t)i * cin + c) * h * w + p];
    std::vector<float> hb(npad, 0.f);
    if (bias) memcpy(hb.data(), bias, (size_t)cout * sizeof(float));
    half_t* dx = s->arena.alloc<half_t>(hx.size()); half_t* dw = s->arena.alloc<half_t>(hw.size());
    float* db = s->arena.alloc<float>(hb.size()); half_t* dy = s->arena.alloc<half_t>((size_t)n * ho * wo * op);
    RT_HIP_CHECK(hipMemcpyAsync(dx, hx.data(), hx.size() * 2, hipMemcpyHostToDevice, s->st));
    RT_HIP_CHECK(hipMemcpyAsync(dw, hw.data(), hw.size() * 2, hipMemcpyHostToDevice, s->st));
    RT_HIP_CHECK(hipMemcpyAsync(db, hb.data(), hb.size() * 4, hipMemcpyHostToDevice, s->st));
    Level Li = make_level(std::vector<std::pair<int, int>>((size_t)n, {h, w})), Lo = make_level(std::vector<std::pair<int, int>>((size_t)n, {ho, wo}));
    const bool flat = kh == 1 && kw == 1 && sh == 1 && sw == 1;   // as the networks run their 1x1 layers: one GEMM over all pixels
    Level Lf = flat ? flat_level(Li) : Level();
    RunCtx c = s->ctx(&s->arena);
    if (flat) upload_levels(c, {&Li, &Lo, &Lf}); else upload_levels(c, {&Li, &Lo});
    nh::Epi16 e; e.bias = db; e.act = act;
    long long* d_st = nullptr;
    const bool stamps = getenv("RT_CONV_STAMPS") != nullptr;
    if (stamps && !nh::conv_stamps_compiled()) fprintf(stderr, "RT_CONV_STAMPS: this library was built without the stamp code (make STAMPS=1): times only\n");
    if (stamps) { d_st = s->arena.alloc<long long>(4096); RT_HIP_CHECK(hipMemsetAsync(d_st, 0, 4096 * 8, s->st)); nh::g_conv_stamps = d_st; }
    hipEvent_t ev0, ev1;
    RT_HIP_CHECK(hipEventCreate(&ev0)); RT_HIP_CHECK(hipEventCreate(&ev1));
    const int reps = stamps ? 5 : 1;
    for (int rep = 0; rep < reps; rep++) {
      if (rep == reps - 1) RT_HIP_CHECK(hipEventRecord(ev0, s->st));
      if (flat) nh::conv16(s->st, dx, cp, Lf.d, Lf.d, 1, 1, Lf.maxW, cp, 1, 1, 1, 1, 0, 0, dw, cout, npad, dy, op, 0, e);
      else nh::conv16(s->st, dx, cp, Li.d, Lo.d, n, Lo.maxH, Lo.maxW, cp, kh, kw, sh, sw, kh / 2, kw / 2, dw, cout, npad, dy, op, 0, e);
    }
    RT_HIP_CHECK(hipEventRecord(ev1, s->st));
    s->sync();
    std::vector<float> hy((size_t)n * ho * wo * op);
    DevBufs::download(hy.data(), dy, hy.size());
    if (!stamps) { (void)hipEventDestroy(ev0); (void)hipEventDestroy(ev1); }
    if (stamps) {
      nh::g_conv_stamps = nullptr;
      std::vector<long long> hs(4096);
      DevBufs::download(hs.data(), d_st, 4096);
      const int nrows = ((cp + 31) / 32) * kh;
      float ms = 0.f;
      RT_HIP_CHECK(hipEventElapsedTime(&ms, ev0, ev1));
      fprintf(stderr, "launch %.3f ms = %.1f TFLOP/s; one workgroup (k_conv16v2): entry->requests %lld, ->data landed %lld, main loop %lld, epilogue %lld ticks (barrier %lld, math + transpose + store issue %lld, store drain %lld)\n",
              ms, 2.0 * n * ho * wo * (double)cout * cin * kh * kw / ms / 1e9, hs[4001] - hs[4000], hs[4002] - hs[4001], hs[4003] - hs[4002], hs[4004] - hs[4003], hs[4005] - hs[4003], hs[4006] - hs[4005], hs[4004] - hs[4006]);
      (void)hipEventDestroy(ev0); (void)hipEventDestroy(ev1);
      fprintf(stderr, "conv16 stamps (s_memtime ticks): stage: t1-t0 | t2-t1 | t3-t2 | t4-t3 | next t0 - t0   (k_conv16: barrier, staging, barrier, MFMAs; k_conv16v2: DMA issue, MFMAs, vmcnt wait, barrier)\n");
      for (int r = 0; r < nrows && r < 790; r++) {
        const long long* t = &hs[(size_t)r * 5];
        const long long nxt = r + 1 < nrows ? hs[(size_t)(r + 1) * 5] : t[4];
        fprintf(stderr, "  %3d: %6lld %6lld %6lld %6lld | %6lld\n", r, t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], nxt - t[0]);
      }
    }
    for (int i = 0; i < n; i++)
      for (int o = 0; o < cout; o++)
        for (int p = 0; p < ho * wo; p++) out[((size_t)i * cout + o) * ho * wo + p] = hy[((size_t)i * ho * wo + p) * op + o];
  });
}
// Kernel micro-benchmark (not part of the drop-in surface): times nn::gemm on random data.
RT_API int rt_bench_gemm(rt_session* s, long long M, int K, int N, int variant, int iters, float* ms_out, float* maxdiff_out) {
  RT_REQUIRE(s && ms_out, s, "rt_bench_gemm: null argument");
  return guarded(s, [&] {
    RT_HIP_CHECK(hipSetDevice(s->device));
    // operand pitches as the networks have them (chan_pitch: 240 -> 256), padding channels zero
    const int Kp = round_up(K, 4), lda = chan_pitch(K), Np = round_up(N, 16), ldc = chan_pitch(N), nkc = (Kp + nn::KC - 1) / nn::KC;
    std::vector<float> ha((size_t)M * lda, 0.f), hw((size_t)nkc * Np * nn::KC, 0.f), hb(Np, 0.1f);
    uint64_t st = 0x2545F4914F6CDD1Dull;   // (xorshift64: 24 live significand bits per value -- the matrix pipe's clock depends on the data)
    auto rnd = [&]() { return (float)((double)(int64_t)(xorshift64(st) >> 11) * (1.0 / 4503599627370496.0)) - 1.0f; };
    for (long long m = 0; m < M; m++) for (int k = 0; k < K; k++) ha[(size_t)m * lda + k] = rnd();
    for (int k = 0; k < K; k++) for (int n = 0; n < N; n++) hw[((size_t)(k / nn::KC) * Np + n) * nn::KC + k % nn::KC] = rnd() * 0.1f;
    DevBufs bufs;
    RestoreInt keep_variant(nn::g_gemm_variant);
    float *dA = bufs.upload(ha.data(), ha.size()), *dW = bufs.upload(hw.data(), hw.size()), *dB = bufs.upload(hb.data(), hb.size()),
          *dC = bufs.zeroed<float>((size_t)M * ldc), *dC0 = bufs.zeroed<float>((size_t)M * ldc);
    ForgetSplit forget{dW};
    Epilogue e{dB, ACT_HSWISH, 1, 1.01f, 0.02f, nullptr, 0};
    nn::g_gemm_variant = 1; nn::gemm(s->st, dA, lda, M, Kp, dW, N, Np, dC0, ldc, 0, e);
    nn::g_gemm_variant = variant;
    timed_and_compared(s->st, iters, [&] { nn::gemm(s->st, dA, lda, M, Kp, dW, N, Np, dC, ldc, 0, e); }, dC0, dC, (size_t)M * ldc, ms_out, maxdiff_out);
  });
}

// Error of one nn::gemm variant against an fp64 product (round 6: the evidence behind the split-bf16 form): random operands with
// FULL 24-bit significands (a few binades each), bias 0, no activation, so the output is the bare product; the first `rows` rows are
// compared with sum_k (double)a * (double)w on the host.  out4 = {max |err|, rms err, max |ref|, rms ref}; variant as rt_bench_gemm
// (1 = narrow fp32-MFMA kernel, 30 = k_gemm32p, 40 = split-bf16).  seed != 0 reseeds the operands; act = an Act value.
RT_API int rt_bench_gemm_err(rt_session* s, long long M, int K, int N, int variant, int rows, int act, unsigned seed, double* out4) {
  RT_REQUIRE(s && out4 && M > 0 && K > 0 && N > 0 && rows > 0, s, "rt_bench_gemm_err: bad argument");
  return guarded(s, [&] {
    RT_HIP_CHECK(hipSetDevice(s->device));
    const int Kp = round_up(K, 4), lda = chan_pitch(K), Np = round_up(N, 16), ldc = chan_pitch(N), nkc = (Kp + nn::KC - 1) / nn::KC;
    std::vector<float> ha((size_t)M * lda, 0.f), hw((size_t)nkc * Np * nn::KC, 0.f), hwd((size_t)K * N), hb(Np, 0.f);
    uint64_t st = 0x9E3779B97F4A7C15ull ^ ((uint64_t)(seed ? seed : 1u) * 0xD1B54A32D192ED03ull);
    // sign * (1 + 23 random bits) * 2^e, e in [-4, 0] (pixels) / [-6, -2] (weights): every significand bit is live
    auto rnd = [&](int e_hi) {
      const uint64_t v = xorshift64(st);
      const uint32_t bits = (uint32_t)((v >> 63) << 31) | (uint32_t)((127 + e_hi - (int)((v >> 40) % 5)) << 23) | (uint32_t)(v & 0x7fffff);
      float f; memcpy(&f, &bits, 4); return f;
    };
    for (long long m = 0; m < M; m++) for (int k = 0; k < K; k++) ha[(size_t)m * lda + k] = rnd(0);
    for (int k = 0; k < K; k++) for (int n = 0; n < N; n++) { const float w = rnd(-2); hwd[(size_t)k * N + n] = w; hw[((size_t)(k / nn::KC) * Np + n) * nn::KC + k % nn::KC] = w; }
    DevBufs bufs;
    RestoreInt keep_variant(nn::g_gemm_variant);
    float *dA = bufs.upload(ha.data(), ha.size()), *dW = bufs.upload(hw.data(), hw.size()), *dB = bufs.upload(hb.data(), hb.size()),
          *dC = bufs.zeroed<float>((size_t)M * ldc);
    ForgetSplit forget{dW};
    Epilogue e; e.bias = dB; e.act = act;
    nn::g_gemm_variant = variant;
    nn::gemm(s->st, dA, lda, M, Kp, dW, N, Np, dC, ldc, 0, e);
    RT_HIP_CHECK(hipStreamSynchronize(s->st));
    // rows from the start, the middle and the end (the last row block is the partial one)
    const long long R = std::min<long long>(rows, M);
    std::vector<float> hc((size_t)R * ldc);
    double max_err = 0, sq_err = 0, max_ref = 0, sq_ref = 0; long long cnt = 0;
    for (int part = 0; part < 3; part++) {
      const long long r0 = part == 0 ? 0 : part == 1 ? std::max<long long>(0, M / 2 - R / 2) : M - R;
      DevBufs::download(hc.data(), dC + r0 * ldc, hc.size());
      std::vector<double> ref(N);
      for (long long m = 0; m < R; m++) {
        std::fill(ref.begin(), ref.end(), 0.0);
        const float* a = &ha[(size_t)(r0 + m) * lda];
        for (int k = 0; k < K; k++) { const double av = a[k]; const float* w = &hwd[(size_t)k * N]; for (int n = 0; n < N; n++) ref[n] += av * (double)w[n]; }
        for (int n = 0; n < N; n++) {
          double rv = ref[n];
          if (act == ACT_HSWISH) rv = rv * std::min(std::max(rv + 3.0, 0.0), 6.0) / 6.0;
          else if (act == ACT_RELU) rv = std::max(rv, 0.0);
          const double d = std::fabs((double)hc[(size_t)m * ldc + n] - rv);
          if (!(d == d)) max_err = INFINITY;
          max_err = std::max(max_err, d); sq_err += d * d; max_ref = std::max(max_ref, std::fabs(rv)); sq_ref += rv * rv; cnt++;
        }
      }
    }
    out4[0] = max_err; out4[1] = std::sqrt(sq_err / cnt); out4[2] = max_ref; out4[3] = std::sqrt(sq_ref / cnt);
  });
}

// One nn::gemm launch on host arrays (tests/test_gpu_ops.py compares it with an fp64 product): the weights packed by the networks'
// pack_linear, the squeeze-excite table built by their se_row_table, the plan of gemm_plan() -- returned with the whole output
// buffer, whose 64 rows past M and columns outside [coff, coff + round_up(N, 4)) must keep the canary.
RT_API int rt_debug_gemm(rt_session* s, const float* A, long long M, int K, int lda, const float* W, int N, const float* bias,
                         int act, int has_lab, float lab_a, float lab_c, const float* residual, int ld_res, const float* se_scale,
                         int ld_scale, const long long* img_rows, int n_img, int se_rows, int ldc, int coff, int variant, int ctc,
                         float* out, int* idx_out, float* prob_out, int* plan_out) {
  RT_REQUIRE(s && A && W && out && plan_out, s, "rt_debug_gemm: null argument");
  RT_REQUIRE(M > 0 && M < (1ll << 30) && K > 0 && N > 0 && lda >= round_up(K, 4) && lda % 4 == 0 && coff >= 0 &&
                 ldc >= coff + round_up(N, 4) && act >= ACT_NONE && act <= ACT_SIGMOID,
             s, "rt_debug_gemm: bad shape");
  RT_REQUIRE(!residual || ld_res >= N, s, "rt_debug_gemm: ld_res < N");
  RT_REQUIRE(!se_scale || (img_rows && n_img > 0 && ld_scale >= round_up(K, 4) && (se_rows == 0 || se_rows == 128 || se_rows == 256)),
             s, "rt_debug_gemm: bad squeeze-excite arguments");
  RT_REQUIRE(ctc >= -1 && ctc <= 2 && (ctc < 0 || (idx_out && prob_out)), s, "rt_debug_gemm: bad ctc arguments");
  long long img_total = 0, min_pix = M;
  for (int i = 0; se_scale && i < n_img; i++) {
    RT_REQUIRE(img_rows[i] > 0, s, "rt_debug_gemm: empty image");
    img_total += img_rows[i]; min_pix = std::min(min_pix, img_rows[i]);
  }
  RT_REQUIRE(!se_scale || img_total == M, s, "rt_debug_gemm: the images' rows do not add up to M");
  return guarded(s, [&] {
    RT_HIP_CHECK(hipSetDevice(s->device));
    WeightStore ws;   // (frees the pack, and the split planes derived from it, on every way out)
    const PackedDense pw = pack_linear(ws, W, bias, K, N);
    DevBufs bufs;
    RestoreInt keep_variant(nn::g_gemm_variant), keep_argmax(nn::g_argmax_wide);
    nn::g_gemm_variant = variant;
    const size_t a_rows = (size_t)M + 256;   // (zero rows past M: a tile's loads stay inside the allocation whatever it reads)
    float* dA = bufs.zeroed<float>(a_rows * lda);
    DevBufs::put(dA, A, (size_t)M * lda);
    const float* dres = residual ? bufs.upload(residual, (size_t)M * ld_res) : nullptr;
    const Lab lab{has_lab, lab_a, lab_c};
    Epilogue e = make_epi(pw, act, &lab, dres, ld_res);
    if (se_scale) {   // as run_lc: the table form the layer asks for (or the one forced), built over consecutive images
      const int tile_rows = se_rows ? se_rows : nn::gemm_se_rows(lda, M, pw.K, N, pw.Npad, act, min_pix);
      if (!tile_rows) throw RtError(RT_ERR_INVALID, "rt_debug_gemm: the layer has no fused squeeze-excite form (gemm_se_rows() == 0)");
      std::vector<int> tab(se_row_table_len(M, tile_rows));
      se_row_table(Ragged(img_rows, n_img).g, M, tile_rows, tab.data());
      e.a_tab = bufs.upload(tab.data(), tab.size()); e.a_tab_stride = tile_rows == 256 ? 3 : 2; e.n_img = n_img;
      e.a_scale = bufs.upload(se_scale, (size_t)n_img * ld_scale); e.ld_scale = ld_scale;
    }
    int* didx = nullptr;
    float* dprob = nullptr;
    if (ctc >= 0) {   // CTC head: per-tile softmax statistics, folded by argmax_merge (SvtrCore::head)
      nn::g_argmax_wide = ctc;
      e.am_tiles = nn::gemm_argmax_tiles(pw.Npad);
      e.am_max = bufs.alloc<float>((size_t)M * e.am_tiles); e.am_idx = bufs.alloc<int>((size_t)M * e.am_tiles);
      e.am_sum = bufs.alloc<float>((size_t)M * e.am_tiles);
      didx = bufs.alloc<int>(M); dprob = bufs.alloc<float>(M);
    }
    const size_t out_n = (size_t)(M + 64) * ldc;
    float* dC = bufs.canary<float>(out_n, s->st);
    const nn::GemmPlan plan = nn::gemm_plan(lda, M, pw.K, N, pw.Npad, ldc, coff, e, stream_cus(s->st));
    nn::gemm(s->st, plan, dA, lda, M, pw.K, pw.w, N, pw.Npad, dC, ldc, coff, e);
    if (ctc >= 0) nn::argmax_merge(s->st, e.am_max, e.am_idx, e.am_sum, e.am_tiles, M, didx, dprob);
    RT_HIP_CHECK(hipStreamSynchronize(s->st));
    DevBufs::download(out, dC, out_n);
    if (ctc >= 0) { DevBufs::download(idx_out, didx, (size_t)M); DevBufs::download(prob_out, dprob, (size_t)M); }
    plan_out[0] = (int)plan.kernel; plan_out[1] = plan.nt; plan_out[2] = plan.kg; plan_out[3] = plan.se; plan_out[4] = plan.bf;
  });
}

// One nn::dwconv launch on host arrays (tests/test_gpu_dwconv_sweep.py): ragged images as the networks' levels lay them out, the
// pooled partial sums in the layout nn::dw_plan gives run_lc, and the channel means k_se_fc makes of them (its walk over
// the partials, without the FCs).  form 0 = k_dwconv_rows, 1 = k_dwconv_sweep where the layer has an instance.
RT_API int rt_debug_dwconv(rt_session* s, const float* x, const int* heights, const int* widths, int n_img, int C, int Cp, int K,
                           int sh, int sw, const float* w, const float* bias, int act, int has_lab, float lab_a, float lab_c,
                           int pooled, int form, float* out, float* partial_out, long long partial_cap, float* mean_out,
                           int* info_out) {
  RT_REQUIRE(s && x && heights && widths && w && bias && out && info_out, s, "rt_debug_dwconv: null argument");
  RT_REQUIRE(n_img > 0 && C > 0 && Cp >= C && Cp % 4 == 0 && (K == 3 || K == 5) && sh >= 1 && sh <= 2 && sw >= 1 && sw <= 2 &&
                 act >= ACT_NONE && act <= ACT_SIGMOID && (form == 0 || form == 1),
             s, "rt_debug_dwconv: bad shape");
  RT_REQUIRE(!pooled || (partial_out && mean_out), s, "rt_debug_dwconv: pooled without buffers for the sums");
  for (int i = 0; i < n_img; i++) RT_REQUIRE(heights[i] > 0 && widths[i] > 0, s, "rt_debug_dwconv: empty image");
  const Ragged gi(heights, widths, n_img), go = gi.down(sh, sw);
  RT_REQUIRE(gi.total * Cp < (1ll << 30), s, "rt_debug_dwconv: too large");
  RestoreInt keep_form(nn::g_dw_sweep);
  nn::g_dw_sweep = form ? 4 : 0;
  const nn::DwPlan plan = nn::dw_plan(K, sh, sw, Cp, go.maxH, go.maxW, pooled != 0);
  const int chunks = pooled ? plan.chunks : 0, strip_R = pooled ? plan.R : 0, spb = pooled ? plan.spb : 0;
  const size_t npart = (size_t)n_img * chunks * Cp;
  RT_REQUIRE(!pooled || (long long)npart <= partial_cap, s, "rt_debug_dwconv: partial_out is too small");
  return guarded(s, [&] {
    RT_HIP_CHECK(hipSetDevice(s->device));
    DevBufs bufs;
    const size_t nout = (size_t)(go.total + 64) * Cp;
    const float *dx = bufs.upload(x, (size_t)gi.total * Cp), *dw = bufs.upload(w, (size_t)K * K * Cp), *db = bufs.upload(bias, (size_t)Cp);
    const ImgGeom *dgi = gi.upload(bufs), *dgo = go.upload(bufs);
    float* dy = bufs.canary<float>(nout, s->st);
    float* dpart = pooled ? bufs.canary<float>(npart, s->st) : nullptr;
    float* dmean = pooled ? bufs.alloc<float>((size_t)n_img * Cp) : nullptr;
    nn::dwconv(s->st, plan, dx, dgi, dgo, n_img, Cp, C, dw, db, act, has_lab, lab_a, lab_c, dy, dpart);
    if (pooled)
      nn::se_fc_from_dw(s->st, dpart, dgo, n_img, chunks, strip_R, spb, C, Cp, nullptr, nullptr, nullptr, nullptr, 0, 0.f, 0, dmean);
    RT_HIP_CHECK(hipStreamSynchronize(s->st));
    DevBufs::download(out, dy, nout);
    if (pooled) { DevBufs::download(partial_out, dpart, npart); DevBufs::download(mean_out, dmean, (size_t)n_img * Cp); }
    info_out[0] = chunks; info_out[1] = strip_R; info_out[2] = spb;
    info_out[3] = plan.kernel == nn::DwKernel::sweep ? 1 : 0;
  });
}

// One nn::attention launch on host arrays: one ImgGeom{off, 1, T} per line, as SvtrCore::mixer passes its token level.
RT_API int rt_debug_attention(rt_session* s, const float* qkv, long long rows, const int* tokens, int n_lines, int heads, float* out) {
  RT_REQUIRE(s && qkv && tokens && out, s, "rt_debug_attention: null argument");
  RT_REQUIRE(rows > 0 && rows < (1ll << 30) && n_lines > 0 && heads > 0 && heads <= 64, s, "rt_debug_attention: bad shape");
  for (int i = 0; i < n_lines; i++) RT_REQUIRE(tokens[i] > 0, s, "rt_debug_attention: a line without tokens");
  const Ragged lines(tokens, n_lines);
  RT_REQUIRE(lines.total == rows, s, "rt_debug_attention: the lines' tokens do not add up to rows");
  return guarded(s, [&] {
    RT_HIP_CHECK(hipSetDevice(s->device));
    const int hd = 15, C = heads * hd;
    DevBufs bufs;
    const float* dq = bufs.upload(qkv, (size_t)rows * 3 * C);
    float* dout = bufs.zeroed<float>((size_t)rows * C);
    nn::attention(s->st, dq, lines.upload(bufs), n_lines, lines.maxW, heads, hd, dout);
    RT_HIP_CHECK(hipStreamSynchronize(s->st));
    DevBufs::download(out, dout, (size_t)rows * C);
  });
}

// The LCNetV3 block of given host weights: packed by the networks' pack_dw / pack_conv (no squeeze-excite, hardswish pointwise tail)
static LcBlock debug_lc_block(WeightStore& ws, int cin, int cout, int sh, int sw, const float* dw_w, const float* dw_bias, const float* pw_w,
                              const float* pw_bias, int dw_act, const Lab& dw_lab, const Lab& pw_lab) {
  LcBlock b;
  b.dw = pack_dw(ws, dw_w, dw_bias, cin, 3); b.dw_lab = dw_lab; b.dw_act = dw_act;
  b.pw = pack_conv(ws, pw_w, pw_bias, cout, cin, 1, 1); b.pw_lab = pw_lab;
  b.sh = sh; b.sw = sw; b.cin = cin; b.cout = cout;
  return b;
}
// The depthwise output buffer run_lc needs from a caller that supplies its own (the unfused route only): zero rows past the last
// pixel, so that a GEMM tile's loads stay inside the allocation (the arena does not clear what it hands out)
static float* debug_lc_mid(DevBufs& bufs, hipStream_t st, const LcBlock& b, const Level& Lo) {
  if (lc_block_plan(b, Lo).route != nn::LC_UNFUSED) return nullptr;
  const size_t nmid = (size_t)(Lo.total + 256) * b.dw.Cp;
  float* dy1 = bufs.alloc<float>(nmid);
  RT_HIP_CHECK(hipMemsetAsync(dy1, 0, nmid * sizeof(float), st));
  return dy1;
}

// One block through the networks' run_lc on host arrays (tests/test_gpu_rec_kernels.py compares it with an fp64 block): a ragged
// batch on the networks' levels, the weights packed by their pack_dw / pack_conv, the kernels of their plan (lc_block_plan, whose
// route is returned).  form = nn::g_lc_wave for the launch.
RT_API int rt_debug_lc_block(rt_session* s, const float* x, const int* heights, const int* widths, int n_img, int cin, int cout,
                             int sh, int sw, const float* dw_w, const float* dw_bias, const float* pw_w, const float* pw_bias,
                             int dw_act, int dw_has_lab, float dw_a, float dw_c, int pw_has_lab, float pw_a, float pw_c, int form,
                             float* out, int* info_out) {
  RT_REQUIRE(s && x && heights && widths && dw_w && dw_bias && pw_w && pw_bias && out && info_out, s, "rt_debug_lc_block: null argument");
  RT_REQUIRE(n_img > 0 && n_img <= RT_MAX_GRID_Y && cin > 0 && cout > 0 && chan_pitch(cin) == round_up(cin, 4) && sh >= 1 && sh <= 2 &&
                 sw >= 1 && sw <= 2 && dw_act >= ACT_NONE && dw_act <= ACT_SIGMOID && (form == 0 || form == 1 || form == 3),
             s, "rt_debug_lc_block: bad shape");
  const int Cp = chan_pitch(cin), ldy = chan_pitch(cout);
  std::vector<std::pair<int, int>> hw;
  for (int i = 0; i < n_img; i++) {
    RT_REQUIRE(heights[i] > 0 && widths[i] > 0, s, "rt_debug_lc_block: empty image");
    hw.push_back({heights[i], widths[i]});
  }
  Level Li = make_level(hw), Lo = down_level(Li, sh, sw);
  RT_REQUIRE(Li.total * Cp < (1ll << 30) && Lo.total * ldy < (1ll << 30), s, "rt_debug_lc_block: too large");
  return guarded(s, [&] {
    s->begin_call();
    WeightStore ws;
    const LcBlock b = debug_lc_block(ws, cin, cout, sh, sw, dw_w, dw_bias, pw_w, pw_bias, dw_act, Lab{dw_has_lab, dw_a, dw_c}, Lab{pw_has_lab, pw_a, pw_c});
    DevBufs bufs;
    RestoreInt keep_form(nn::g_lc_wave);
    nn::g_lc_wave = form;
    RunCtx c = s->ctx(&s->arena);
    upload_levels(c, {&Li, &Lo});
    const size_t nin = (size_t)Li.total * Cp, nout = (size_t)(Lo.total + 64) * ldy;   // (64 canary rows past the last image)
    const float* dx = bufs.upload(x, nin);
    float* dy = bufs.canary<float>(nout, s->st);
    run_lc(c, b, dx, Li, Lo, dy, debug_lc_mid(bufs, s->st, b, Lo));
    RT_HIP_CHECK(hipStreamSynchronize(s->st));
    DevBufs::download(out, dy, nout);
    info_out[0] = (int)lc_block_plan(b, Lo).route;
  });
}

// The fields of nn::dw_plan() for a K x K depthwise conv, stride (sh, sw), pitch Cp, onto images of at most maxHo x maxWo output
// pixels, under g_dw_sweep = form ? 4 : 0 -- the plan rt_debug_dwconv launches by.  Host only: no session, no device.
// plan_out[8] = {DwKernel value (lc_plan.h), inst, R, lanes, spb, chunks, grid_x, grid_z}.
RT_API int rt_debug_dw_plan(int K, int sh, int sw, int Cp, int maxHo, int maxWo, int pooled, int form, int* plan_out) {
  rt_session* const none = nullptr;
  RT_REQUIRE(plan_out, none, "rt_debug_dw_plan: null argument");
  RT_REQUIRE(Cp > 0 && Cp % 4 == 0 && maxHo > 0 && maxWo > 0 && (form == 0 || form == 1), none, "rt_debug_dw_plan: bad shape");
  RestoreInt keep_form(nn::g_dw_sweep);
  nn::g_dw_sweep = form ? 4 : 0;
  const nn::DwPlan p = nn::dw_plan(K, sh, sw, Cp, maxHo, maxWo, pooled != 0);
  const int f[8] = {(int)p.kernel, p.inst, p.R, p.lanes, p.spb, p.chunks, (int)p.grid_x, (int)p.grid_z};
  memcpy(plan_out, f, sizeof f);
  return RT_OK;
}

// One wide LCNetV3 block (K x K depthwise [-> squeeze-excite] -> 1x1 conv + hardswish) through the networks' run_lc on host arrays
// (tests/test_gpu_dw_kernels.py compares it with an fp64 block): what rt_debug_lc_block cannot express -- K = 5, squeeze-excite
// weights (the host-array get_se, b.se = true), the depthwise form (g_dw_sweep) under GEMM variant 0, and the depthwise buffer y1
// handed to run_lc returned beside the output.  What ran is reported from run_lc's own plan and trace, not recomputed.  Every
// argument is checked with its own message before any device work; the session is looked at last.
RT_API int rt_debug_lc_wide(rt_session* s, const float* x, const int* heights, const int* widths, int n_img, int K, int cin, int cout,
                            int sh, int sw, const float* dw_w, const float* dw_bias, const float* pw_w, const float* pw_bias, int dw_act,
                            int dw_has_lab, float dw_a, float dw_c, int pw_has_lab, float pw_a, float pw_c, const float* fc1_w,
                            const float* fc1_b, const float* fc2_w, const float* fc2_b, int dw_form, float* out, long long out_len,
                            float* y1_out, long long y1_len, float* scale_out, long long scale_len, int* info_out) {
  RT_REQUIRE(x && heights && widths && dw_w && dw_bias && pw_w && pw_bias && out && y1_out && info_out, s, "rt_debug_lc_wide: null argument");
  const bool se = fc1_w || fc1_b || fc2_w || fc2_b;
  RT_REQUIRE(!se || (fc1_w && fc1_b && fc2_w && fc2_b && scale_out), s, "rt_debug_lc_wide: a squeeze-excite block needs both FCs and scale_out");
  RT_REQUIRE(n_img > 0 && n_img <= 4096, s, "rt_debug_lc_wide: bad image count");
  RT_REQUIRE(cin > 0 && cin <= 512 && cin % 4 == 0 && cout > 0 && cout <= 960, s, "rt_debug_lc_wide: bad channel counts (cin a multiple of 4 up to 512, cout up to 960)");
  RT_REQUIRE((K == 3 || K == 5) && sh >= 1 && sh <= 2 && sw >= 1 && sw <= 2 && dw_act >= ACT_NONE && dw_act <= ACT_SIGMOID &&
                 (dw_form == 0 || dw_form == 1), s, "rt_debug_lc_wide: no such block (K 3 or 5, strides 1 or 2, dw_form 0 or 1)");
  for (int i = 0; i < n_img; i++)
    RT_REQUIRE(heights[i] > 0 && widths[i] > 0 && heights[i] <= 4096 && widths[i] <= 65536, s, "rt_debug_lc_wide: empty or oversized image");
  const int Cp = chan_pitch(cin), ldy = chan_pitch(cout);
  const Ragged gi(heights, widths, n_img), go = gi.down(sh, sw);
  RT_REQUIRE(gi.total * Cp < (1ll << 28) && go.total * ldy < (1ll << 28), s, "rt_debug_lc_wide: too large");
  const long long out_n = (go.total + 64) * ldy, y1_n = (go.total + 64) * Cp, scale_n = se ? (long long)(n_img + 64) * Cp : 0;
  RT_REQUIRE(out_len == out_n && y1_len == y1_n, s, "rt_debug_lc_wide: out or y1_out has the wrong length");
  RT_REQUIRE(scale_len == scale_n, s, "rt_debug_lc_wide: scale_out has the wrong length");
  RT_REQUIRE(s, s, "rt_debug_lc_wide: null session");
  return guarded(s, [&] {
    s->begin_call();
    WeightStore ws;
    LcBlock b;
    b.dw = pack_dw(ws, dw_w, dw_bias, cin, K); b.dw_lab = Lab{dw_has_lab, dw_a, dw_c}; b.dw_act = dw_act;
    b.se = se;
    if (se) b.sew = get_se(ws, fc1_w, fc1_b, fc2_w, fc2_b, cin, cin / 4);
    b.pw = pack_conv(ws, pw_w, pw_bias, cout, cin, 1, 1); b.pw_lab = Lab{pw_has_lab, pw_a, pw_c};
    b.sh = sh; b.sw = sw; b.cin = cin; b.cout = cout;
    std::vector<std::pair<int, int>> hw;
    for (int i = 0; i < n_img; i++) hw.push_back({heights[i], widths[i]});
    Level Li = make_level(hw), Lo = down_level(Li, sh, sw);
    DevBufs bufs;
    RestoreInt keep_form(nn::g_dw_sweep), keep_variant(nn::g_gemm_variant);
    nn::g_dw_sweep = dw_form ? 4 : 0;
    nn::g_gemm_variant = 0;   // (a forced variant takes no folded squeeze-excite form)
    RunCtx c = s->ctx(&s->arena);
    upload_levels(c, {&Li, &Lo});
    const float* dx = bufs.upload(x, (size_t)Li.total * Cp);
    float* dy = bufs.canary<float>((size_t)out_n, s->st);
    // y1: 256 rows past the last pixel, as a GEMM tile reads past the end of its A rows (rows are independent: what they hold
    // reaches no stored output); the first 64 of them are returned and must keep the canary
    float* dy1 = bufs.canary<float>((size_t)(Lo.total + 256) * Cp, s->st);
    const nn::LcPlan plan = lc_block_plan(b, Lo);
    LcTrace tr;
    run_lc(c, b, dx, Li, Lo, dy, dy1, &tr);
    RT_HIP_CHECK(hipStreamSynchronize(s->st));
    DevBufs::download(out, dy, (size_t)out_n);
    DevBufs::download(y1_out, dy1, (size_t)y1_n);
    if (se) {   // the scales [n_img][Cp], then 64 rows of the canary as the other buffers have them
      const uint32_t cw = RT_DEBUG_CANARY;
      for (long long i = 0; i < scale_n; i++) memcpy(scale_out + i, &cw, 4);
      if (tr.scale) DevBufs::download(scale_out, tr.scale, (size_t)n_img * Cp);
    }
    const bool unfused = plan.route == nn::LC_UNFUSED;
    const int f[16] = {(int)plan.route, unfused ? (int)plan.dw.kernel : 0, unfused ? plan.dw.inst : plan.inst, plan.dw.R, plan.dw.lanes,
                       plan.dw.spb, plan.dw.chunks, (int)plan.dw.grid_x, (int)plan.dw.grid_z, plan.se_rows,
                       unfused ? (int)tr.gemm.kernel : 0, unfused && tr.gemm.se ? 1 : 0, tr.scale ? (tr.scaled_in_place ? 2 : 1) : 0, 0, 0, 0};
    memcpy(info_out, f, sizeof f);
  });
}

// One 1x3 token conv on host arrays: form 0 = nn::conv_sp on one ImgGeom{off, 1, T} per line (the fallback of RecNet::run), form 1 =
// nn::conv13_flat over the flat list with RecNet's token_line_flags; the weights through pack_conv.
RT_API int rt_debug_conv13(rt_session* s, const float* x, long long rows, int ldx, const int* tokens_per_line, int n_lines, int cin,
                           const float* w, int cout, const float* bias, int act, int form, float* out, int* info_out) {
  RT_REQUIRE(s && x && tokens_per_line && w && out && info_out, s, "rt_debug_conv13: null argument");
  RT_REQUIRE(rows > 0 && rows < (1ll << 24) && n_lines > 0 && n_lines <= RT_MAX_GRID_Y && cin > 0 && cin % 4 == 0 && ldx >= cin &&
                 ldx % 4 == 0 && cout > 0 && cout <= 64 && act >= ACT_NONE && act <= ACT_SIGMOID && (form == 0 || form == 1),
             s, "rt_debug_conv13: bad shape");
  RT_REQUIRE(rows * ldx < (1ll << 30), s, "rt_debug_conv13: too large");
  for (int i = 0; i < n_lines; i++) RT_REQUIRE(tokens_per_line[i] > 0, s, "rt_debug_conv13: a line without tokens");
  const Ragged lines(tokens_per_line, n_lines);
  RT_REQUIRE(lines.total == rows, s, "rt_debug_conv13: the lines' tokens do not add up to rows");
  return guarded(s, [&] {
    RT_HIP_CHECK(hipSetDevice(s->device));
    WeightStore ws;
    const PackedDense pw = pack_conv(ws, w, bias, cout, cin, 1, 3);
    if (form == 1 && !nn::conv13_flat_supported(cout, pw.Npad)) throw RtError(RT_ERR_INVALID, "rt_debug_conv13: conv13_flat has no instance for the layer");
    const Epilogue e = make_epi(pw, act);
    const int ldy = chan_pitch(cout);
    DevBufs bufs;
    const size_t nin = (size_t)rows * ldx, nout = (size_t)(rows + 64) * ldy;
    const float* dx = bufs.upload(x, nin);
    float* dy = bufs.canary<float>(nout, s->st);
    info_out[0] = 0; info_out[1] = stream_cus(s->st);
    if (form == 1) {
      std::vector<unsigned char> hf((size_t)rows);
      token_line_flags(lines.g, rows, hf.data());
      const unsigned char* df = bufs.upload(hf.data(), (size_t)rows);
      info_out[0] = nn::conv13_flat_nt(rows, pw.Npad, info_out[1]);
      nn::conv13_flat(s->st, dx, ldx, rows, df, cin, pw.w, cout, pw.Npad, dy, ldy, e);
    } else {
      nn::conv_sp(s->st, 1, 3, dx, ldx, lines.upload(bufs), n_lines, 1, lines.maxW, cin, pw.w, cout, pw.Npad, dy, ldy, e);
    }
    RT_HIP_CHECK(hipStreamSynchronize(s->st));
    DevBufs::download(out, dy, nout);
  });
}

// One nn::add_layernorm launch on host arrays.
RT_API int rt_debug_layernorm(rt_session* s, const float* x, const float* r, long long rows, int C, const float* g,
                              const float* beta, float eps, float* out) {
  RT_REQUIRE(s && x && g && beta && out, s, "rt_debug_layernorm: null argument");
  RT_REQUIRE(rows > 0 && rows < (1ll << 22) && C > 0 && C <= 256 && eps > 0.f, s, "rt_debug_layernorm: bad shape");
  return guarded(s, [&] {
    RT_HIP_CHECK(hipSetDevice(s->device));
    DevBufs bufs;
    const size_t nin = (size_t)rows * C, nout = (size_t)(rows + 64) * C;
    const float *dx = bufs.upload(x, nin), *dr = r ? bufs.upload(r, nin) : nullptr, *dg = bufs.upload(g, (size_t)C), *db = bufs.upload(beta, (size_t)C);
    float* dy = bufs.canary<float>(nout, s->st);
    nn::add_layernorm(s->st, dx, dr, rows, C, dg, db, eps, dy);
    RT_HIP_CHECK(hipStreamSynchronize(s->st));
    DevBufs::download(out, dy, nout);
  });
}

// One launch of a glue kernel of the fp16 family (nn_f16.hip) on host arrays, for tests/test_gpu_f16_kernels.py: ragged source
// and destination image lists laid out as the networks' levels are, operands given as the rows of the buffers the networks
// pass (so views into concat buffers are a pitch and a channel offset), the output buffer canary-filled with 64 spare rows.
// Everything a kernel may address is checked against the lengths the caller gives before any device work.
namespace {
enum Glue16Op { G16_DWCONV = 0, G16_GLOBAL_MEAN, G16_GATE, G16_SCALE_CHANNELS, G16_UPSAMPLE_ADD, G16_UPSAMPLE_INTO, G16_MAXPOOL,
                G16_AVGPOOL, G16_PIXEL_SHUFFLE, G16_DECONV_TO_MAP, G16_MAP_WINDOW, G16_U8_TO_H8, G16_F32X4_TO_H8, G16_H_TO_F32,
                G16_F32_TO_H, G16_COUNT };
}  // namespace
RT_API int rt_debug_glue16(rt_session* s, int op, const int* ip, const float* fp, const int* src_h, const int* src_w,
                           const int* dst_h, const int* dst_w, int n_img, const float* x, long long x_len, const float* x2,
                           long long x2_len, const float* tab, long long tab_len, float* out, long long out_len) {
  // (the session is looked at last: without a device there is none, and the argument checks can still be told apart by their messages)
  RT_REQUIRE(ip && fp && src_h && src_w && dst_h && dst_w && x && out, s, "rt_debug_glue16: null argument");
  RT_REQUIRE(op >= 0 && op < G16_COUNT && n_img > 0 && n_img <= 4096, s, "rt_debug_glue16: bad op or image count");
  const int C = ip[0], ldx = ip[1], xoff = ip[2], ldy = ip[3], yoff = ip[4];
  RT_REQUIRE(C > 0 && C <= 4096 && ldx > 0 && ldx <= 8192 && ldy > 0 && ldy <= 8192 && xoff >= 0 && yoff >= 0, s, "rt_debug_glue16: bad channel counts");
  for (int i = 0; i < n_img; i++)
    RT_REQUIRE(src_h[i] > 0 && src_w[i] > 0 && dst_h[i] > 0 && dst_w[i] > 0 && src_h[i] < 32768 && src_w[i] < 32768 && dst_h[i] < 32768 && dst_w[i] < 32768,
               s, "rt_debug_glue16: empty or oversized image");
  const Ragged gs(src_h, src_w, n_img), gd(dst_h, dst_w, n_img);
  const long long ps = gs.total, pd = gd.total, max_s = gs.max_pix, max_d = gd.max_pix;
  RT_REQUIRE(ps * ldx < (1ll << 28) && pd * ldy < (1ll << 28), s, "rt_debug_glue16: too large");
  // what the op reads and writes: x / x2 / tab lengths in floats, the output's rows, pitch and type
  const bool vec = op != G16_GATE && op != G16_H_TO_F32 && op != G16_F32_TO_H;   // 16-byte vectors of 8 halves
  bool x_half = true, out_half = true, in_place = false;
  long long x_need = ps * ldx, x2_need = 0, tab_need = 0, out_rows = pd;
  int out_ld = ldy, c_read = C, c_write = C;
  bool ok = true;
  switch (op) {
    case G16_DWCONV: {
      const int K = ip[5], sh = ip[6], sw = ip[7];
      ok = (K == 3 || K == 5) && sh >= 1 && sh <= 2 && sw >= 1 && sw <= 2 && ip[8] >= ACT_NONE && ip[8] <= ACT_SIGMOID;
      for (int i = 0; ok && i < n_img; i++) ok = dst_h[i] == (src_h[i] + sh - 1) / sh && dst_w[i] == (src_w[i] + sw - 1) / sw;
      tab_need = ok ? (long long)(K * K + 1) * C : 0;
    } break;
    case G16_GLOBAL_MEAN: out_half = false; out_rows = n_img; ok = ldy == C && yoff == 0; break;
    case G16_GATE: x_half = false; out_half = false; x_need = (long long)n_img * ldx; out_rows = n_img; c_write = ldy; ok = ldy >= C && yoff == 0 && (ip[5] == 0 || ip[5] == 1); break;
    case G16_SCALE_CHANNELS:
      in_place = ip[7] != 0; tab_need = (long long)n_img * C;
      ok = ip[5] >= 0 && ip[5] <= 8192 && ip[5] % 8 == 0 && ip[6] >= 0 && ip[6] % 8 == 0 && (ip[5] == 0 || ip[6] + C <= ip[5]) && (!in_place || ldx == ldy);
      for (int i = 0; ok && i < n_img; i++) ok = dst_h[i] == src_h[i] && dst_w[i] == src_w[i];
      x2_need = ps * ip[5];
      break;
    case G16_UPSAMPLE_ADD:
      in_place = ip[5] != 0; tab_need = ip[6] ? (long long)n_img * C : 0; x2_need = pd * C;
      ok = ldx == C && ldy == C && xoff == 0 && yoff == 0;
      break;
    case G16_UPSAMPLE_INTO: ok = ip[5] >= 0 && ip[5] <= 3 && (ip[6] == 0 || (ip[6] >= C && ip[6] <= 8192)); tab_need = (long long)n_img * ip[6]; break;
    case G16_MAXPOOL:
      ok = ip[5] >= 1 && ip[5] <= 5 && ip[6] >= 1 && ip[6] <= 5 && ip[7] >= 1 && ip[7] <= 4 && ip[8] >= 1 && ip[8] <= 4 && ip[9] >= 0 && ip[9] < ip[5] && ip[10] >= 0 && ip[10] < ip[6];
      break;
    case G16_AVGPOOL:   // (window = stride, no padding: the kernel reads every tap unchecked)
      ok = ip[5] >= 1 && ip[5] <= 8 && ip[6] >= 1 && ip[6] <= 8;
      for (int i = 0; ok && i < n_img; i++) ok = (long long)dst_h[i] * ip[5] <= src_h[i] && (long long)dst_w[i] * ip[6] <= src_w[i];
      break;
    case G16_PIXEL_SHUFFLE:
      c_read = 4 * C;
      for (int i = 0; ok && i < n_img; i++) ok = dst_h[i] <= 2 * src_h[i] && dst_w[i] <= 2 * src_w[i];
      break;
    case G16_DECONV_TO_MAP:
      out_half = false; out_ld = 1; c_write = 1; tab_need = 4ll * C; ok = ldy == 1 && yoff == 0;
      for (int i = 0; ok && i < n_img; i++) ok = dst_h[i] == 2 * src_h[i] && dst_w[i] == 2 * src_w[i];
      break;
    case G16_MAP_WINDOW: x_half = false; x_need = ps; c_read = 1; c_write = 16; ok = ldx == 1 && xoff == 0 && C == 16; break;
    case G16_U8_TO_H8:
      x_half = false; x_need = ps * 3; c_read = 3; c_write = 8; ok = ldx == 3 && xoff == 0 && ldy == 8 && yoff == 0 && C == 8;
      for (int i = 0; ok && i < n_img; i++) ok = (long long)dst_h[i] * dst_w[i] >= (long long)src_h[i] * src_w[i];
      break;
    case G16_F32X4_TO_H8: x_half = false; x_need = ps * 4; c_read = 4; c_write = 8; out_rows = ps; ok = ldx == 4 && xoff == 0 && ldy == 8 && yoff == 0 && C == 8; break;
    case G16_H_TO_F32: out_half = false; out_rows = ps; break;
    case G16_F32_TO_H: x_half = false; out_rows = ps; break;
  }
  RT_REQUIRE(ok, s, "rt_debug_glue16: bad parameters for the op");
  RT_REQUIRE(xoff + c_read <= ldx && yoff + c_write <= out_ld, s, "rt_debug_glue16: the channel window leaves the row");
  RT_REQUIRE(!vec || ((!x_half || (ldx % 8 == 0 && xoff % 8 == 0)) && (!out_half || (out_ld % 8 == 0 && yoff % 8 == 0)) && C % 8 == 0),
             s, "rt_debug_glue16: channel counts, pitches and offsets must be multiples of 8");
  const long long out_n = (out_rows + 64) * out_ld;
  RT_REQUIRE(x_len >= x_need && out_len == out_n, s, "rt_debug_glue16: x is too short or out has the wrong length");
  RT_REQUIRE((x2_need == 0 || (x2 && x2_len >= x2_need)) && (tab_need == 0 || (tab && tab_len >= tab_need)), s, "rt_debug_glue16: x2 or tab is missing or too short");
  RT_REQUIRE(s, s, "rt_debug_glue16: null session");
  return guarded(s, [&] {
    RT_HIP_CHECK(hipSetDevice(s->device));
    DevBufs bufs;
    hipStream_t st = s->st;
    const ImgGeom *dgs = gs.upload(bufs), *dgd = gd.upload(bufs);
    void* dout = out_half ? (void*)bufs.canary<half_t>((size_t)out_n, st) : (void*)bufs.canary<float>((size_t)out_n, st);
    half_t* yh = (half_t*)dout; float* yf = (float*)dout;
    const float* first = in_place ? (op == G16_UPSAMPLE_ADD ? x2 : x) : nullptr;   // the operand that is also the output
    if (first) put_as(yh, first, (size_t)(op == G16_UPSAMPLE_ADD ? x2_need : x_need));
    const half_t* xh = nullptr; const float* xf = nullptr;
    if (op == G16_U8_TO_H8) {}
    else if (in_place && op == G16_SCALE_CHANNELS) xh = yh;
    else if (x_half) xh = upload_as<half_t>(bufs, x, (size_t)x_need);
    else xf = upload_as<float>(bufs, x, (size_t)x_need);
    const half_t* x2h = nullptr;
    if (x2_need) x2h = (in_place && op == G16_UPSAMPLE_ADD) ? yh : upload_as<half_t>(bufs, x2, (size_t)x2_need);
    const float* dtab = (tab_need && op != G16_DWCONV) ? upload_as<float>(bufs, tab, (size_t)tab_need) : nullptr;
    switch (op) {
      case G16_DWCONV: {
        const int K = ip[5];
        const half_t* dw = upload_as<half_t>(bufs, tab, (size_t)K * K * C);
        const float* db = upload_as<float>(bufs, tab + (size_t)K * K * C, (size_t)C);
        nh::dwconv16(st, K, ip[6], ip[7], xh + xoff, ldx, dgs, dgd, n_img, gd.maxH, gd.maxW, C, dw, db, ip[8], ip[9], fp[0], fp[1], yh + yoff, ldy);
      } break;
      case G16_GLOBAL_MEAN: {
        float* partial = bufs.alloc<float>((size_t)n_img * nh::pool_chunks16(max_s) * C);
        nh::global_mean16(st, xh + xoff, ldx, dgs, n_img, max_s, C, partial, yf);
      } break;
      case G16_GATE: nh::gate16(st, xf + xoff, ldx, n_img, C, ldy, fp[0], ip[5], yf); break;
      case G16_SCALE_CHANNELS:
        nh::scale_channels16(st, xh + xoff, ldx, dgs, n_img, max_s, C, dtab, ip[5] ? x2h + ip[6] : nullptr, ip[5], yh + yoff, ldy);
        break;
      case G16_UPSAMPLE_ADD: nh::upsample_add16(st, x2h, xh, dgd, dgs, n_img, max_d, C, yh, ip[6] ? dtab : nullptr); break;
      case G16_UPSAMPLE_INTO: nh::upsample_into16(st, xh + xoff, ldx, dgs, dgd, n_img, max_d, C, ip[5], yh, ldy, yoff, ip[6] ? dtab : nullptr, ip[6]); break;
      case G16_MAXPOOL: nh::maxpool16(st, xh + xoff, ldx, dgs, dgd, n_img, max_d, C, ip[5], ip[6], ip[7], ip[8], ip[9], ip[10], yh + yoff, ldy); break;
      case G16_AVGPOOL: nh::avgpool16(st, xh + xoff, ldx, dgs, dgd, n_img, max_d, C, ip[5], ip[6], yh + yoff, ldy); break;
      case G16_PIXEL_SHUFFLE: nh::pixel_shuffle16(st, xh + xoff, ldx, dgs, dgd, n_img, max_d, C, yh, ldy, yoff); break;
      case G16_DECONV_TO_MAP: nh::deconv_to_map16(st, xh + xoff, ldx, dgs, dgd, n_img, max_s, C, dtab, fp[0], yf); break;
      case G16_MAP_WINDOW: nh::map_window16(st, xf, dgs, dgd, n_img, max_d, yh, ldy, yoff); break;
      case G16_U8_TO_H8: {
        const uint8_t* d8 = upload_as<uint8_t>(bufs, x, (size_t)x_need);
        std::vector<nh::U8Page16> pages(n_img);
        for (int i = 0; i < n_img; i++) pages[i] = nh::U8Page16{d8 + gs.g[i].off * 3, (long long)gs.g[i].H * gs.g[i].W, gd.g[i].off};
        nh::u8_to_h8(st, bufs.upload(pages.data(), pages.size()), n_img, max_s, fp[0], fp + 1, fp + 4, yh);
      } break;
      case G16_F32X4_TO_H8: nh::f32x4_to_h8(st, xf, ps, yh); break;
      case G16_H_TO_F32: nh::h_to_f32(st, xh + xoff, ldx, ps, C, yf, ldy, yoff); break;
      case G16_F32_TO_H: nh::f32_to_h(st, xf + xoff, ldx, ps, C, yh, ldy, yoff); break;
    }
    RT_HIP_CHECK(hipStreamSynchronize(st));
    if (out_half) DevBufs::download(out, yh, (size_t)out_n); else DevBufs::download(out, yf, (size_t)out_n);
  });
}

// One launch of a kernel of the fp32 det neck / head on host arrays, for tests/test_gpu_fpn_kernels.py (include/retto_hip.h lists
// the ops and their operand slots): the launchers of nn.h as DetNet::run issues them, the weights through the packers DetNet's
// constructor calls.  Every address a kernel can form is checked against the callers' lengths first; the session is looked at last.
namespace {
enum FpnOp { FPN_PHASE = 0, FPN_CLASS, FPN_COMPOSE, FPN_TAIL, FPN_LATERAL_ADD, FPN_UPSAMPLE_ADD, FPN_SE_PROJECTED, FPN_SE_TILES,
             FPN_HEAD_FUSED, FPN_CONV3, FPN_COUNT };
constexpr int FPN_IN = 10, FPN_OUT = 3;
}  // namespace
RT_API int rt_debug_fpn(rt_session* s, int op, const int* ip, const float* fp, const int* fine_h, const int* fine_w,
                        const int* coarse_h, const int* coarse_w, int n_img, const float* const* in, const long long* in_len,
                        float* const* out, const long long* out_len, int* info_out) {
  RT_REQUIRE(ip && fp && fine_h && fine_w && coarse_h && coarse_w && in && in_len && out && out_len && info_out, s, "rt_debug_fpn: null argument");
  RT_REQUIRE(op >= 0 && op < FPN_COUNT && n_img > 0 && n_img <= 256, s, "rt_debug_fpn: bad op or image count");
  // the levels: 0 = fine, 1 = coarse (given), 2 / 3 = half of the one before (derived, where the op reads them)
  for (int i = 0; i < n_img; i++)
    RT_REQUIRE(fine_h[i] > 0 && fine_w[i] > 0 && coarse_h[i] > 0 && coarse_w[i] > 0 && fine_h[i] <= 4096 && fine_w[i] <= 4096 &&
                   coarse_h[i] <= 4096 && coarse_w[i] <= 4096, s, "rt_debug_fpn: empty or oversized image");
  Ragged lv[4] = {Ragged(fine_h, fine_w, n_img)};
  const int maxH = lv[0].maxH, maxW = lv[0].maxW;
  const bool has_coarse = op == FPN_PHASE || op == FPN_UPSAMPLE_ADD || op == FPN_HEAD_FUSED || (op == FPN_CLASS && (ip[1] & 4)) ||
                          (op == FPN_LATERAL_ADD && ip[1]);
  const int n_levels = op == FPN_HEAD_FUSED ? 4 : (op == FPN_PHASE && (ip[2] & 8)) ? 3 : has_coarse ? 2 : 1;
  for (int l = 1; l < n_levels; l++) {   // (a halved level is down(2, 2) exactly: the check below leaves even extents only)
    lv[l] = l == 1 ? Ragged(coarse_h, coarse_w, n_img) : lv[l - 1].down(2, 2);
    for (int i = 0; i < n_img; i++)
      RT_REQUIRE(lv[l].g[i].H > 0 && lv[l].g[i].W > 0 && lv[l - 1].g[i].H == 2 * lv[l].g[i].H && lv[l - 1].g[i].W == 2 * lv[l].g[i].W, s,
                 "rt_debug_fpn: a level that is not exactly twice the next coarser one");
  }
  RT_REQUIRE(lv[0].total < (1ll << 20), s, "rt_debug_fpn: too large");
  const long long pf = lv[0].total, pc = lv[1].total;
  const int tiles = ((maxW + 15) / 16) * ((maxH + 15) / 16);
  // what the op reads (floats per slot; 0 = unused) and writes (rows and pitch per output)
  long long need[FPN_IN] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, out_rows[FPN_OUT] = {0, 0, 0};
  int out_ld[FPN_OUT] = {0, 0, 0};
  const long long W33 = 24ll * 96 * 9;
  bool ok = true, inst = true;
  int cin = 0, cf = 0, flags = 0;
  switch (op) {
    case FPN_PHASE: {
      cin = ip[0]; cf = round_up(std::max(cin, 1), 4); flags = ip[2];
      const int cc = ip[1];
      const bool head = cin == 24;
      ok = cin > 0 && cin <= 24 && cc > 0 && cc <= 96 && flags >= 0 && flags < 128 && !((flags & 8) && (flags & 1));
      // (what DetNet::run passes: the tap tensors of 12 / 18 channels over a 96-channel level, the head's 24 over 24)
      inst = ok && (cin == 12 || cin == 18 || cin == 24) && cc == (head ? 24 : 96) && nn::fpn_phase_instance(cin, cc, (flags & 8) != 0) != 0 &&
             (head ? !(flags & 64) : !(flags & (8 | 16 | 32)));
      if (!ok || !inst) break;
      need[0] = pf * cf; need[1] = pc * cc; need[2] = W33; need[3] = (flags & 1) ? 24 : 0;
      need[4] = (!head && !(flags & 64)) ? (long long)n_img * 216 * cf : 0;
      need[5] = (flags & 64) ? 96ll * cin : 0; need[6] = (flags & 64) ? (long long)n_img * 96 : 0;
      need[7] = (flags & 16) ? (long long)n_img * 24 : 0; need[8] = (flags & 32) ? (long long)n_img * 24 : 0;
      need[9] = (flags & 8) ? 9 * lv[2].total * 24 : 0;
      out_rows[0] = pf; out_ld[0] = 24;
      if (flags & 2) { out_rows[1] = (long long)n_img * tiles; out_ld[1] = 24; }
      if (flags & 64) { out_rows[2] = (long long)n_img * 216; out_ld[2] = cf; }
    } break;
    case FPN_CLASS:
      flags = ip[1];
      ok = ip[0] >= 0 && ip[0] <= 72 && ip[0] % 24 == 0 && flags >= 0 && flags < 8;
      need[0] = pf * 24; need[1] = W33; need[2] = (flags & 1) ? 24 : 0; need[3] = (flags & 2) ? (long long)n_img * 24 : 0;
      need[4] = (flags & 4) ? 9 * pc * 24 : 0;
      out_rows[0] = 9 * pf; out_ld[0] = 24;
      break;
    case FPN_COMPOSE:
      cin = ip[0]; cf = round_up(std::max(cin, 1), 4);
      ok = cin > 0 && cin <= 24;
      inst = ok && (cin == 12 || cin == 18) && nn::fpn_phase_instance(cin, 96, false) != 0;
      need[0] = 96ll * cin; need[1] = (long long)n_img * 96; need[2] = W33;
      out_rows[0] = (long long)n_img * 216; out_ld[0] = cf;
      break;
    case FPN_TAIL:
      need[0] = pf * 24; need[1] = 24 * 24 * 4; need[2] = 24; need[3] = 24 * 4; need[4] = 1;
      out_rows[0] = 16 * pf; out_ld[0] = 1;
      break;
    case FPN_LATERAL_ADD:
      cin = ip[0]; cf = round_up(std::max(cin, 1), 4);
      ok = cin > 0 && cin <= 64 && (ip[1] == 0 || ip[1] == 1);
      need[0] = pf * cf; need[1] = 96ll * cin; need[2] = (long long)n_img * 96; need[3] = ip[1] ? pc * 96 : 0;
      out_rows[0] = pf; out_ld[0] = 96;
      break;
    case FPN_UPSAMPLE_ADD:
      ok = (ip[0] == 0 || ip[0] == 1) && (ip[1] == 0 || ip[1] == 1);
      need[0] = pf * 96; need[1] = pc * 96; need[2] = ip[1] ? (long long)n_img * 96 : 0;
      out_rows[0] = pf; out_ld[0] = 96;
      break;
    case FPN_SE_PROJECTED:
      cin = ip[0]; cf = round_up(std::max(cin, 1), 4);
      ok = cin > 0 && cin <= 64 && ip[1] > 0 && ip[1] <= 96 && (ip[2] == 0 || ip[2] == 1) && fp[0] > 0.f && fp[0] <= 1.f;
      need[0] = pf * cf; need[1] = 96ll * cin; need[2] = 96ll * ip[1]; need[3] = ip[1]; need[4] = 96ll * ip[1]; need[5] = 96;
      out_rows[0] = n_img; out_ld[0] = 96;
      break;
    case FPN_SE_TILES:
      ok = ip[0] > 0 && ip[0] <= 24 && (ip[1] == 0 || ip[1] == 1) && fp[0] > 0.f && fp[0] <= 1.f;
      need[0] = (long long)n_img * tiles * 24; need[1] = 24ll * ip[0]; need[2] = ip[0]; need[3] = 24ll * ip[0]; need[4] = 24;
      out_rows[0] = n_img; out_ld[0] = 24;
      break;
    case FPN_HEAD_FUSED:
      flags = ip[0];
      ok = flags >= 0 && flags < 64;
      for (int l = 0; l < 4; l++) { need[l] = lv[3 - l].total * 24; need[6 + l] = (flags & (1 << l)) ? (long long)n_img * 24 : 0; }
      need[4] = W33; need[5] = (flags & 16) ? 24 : 0;
      out_rows[0] = pf; out_ld[0] = 24;
      break;
    case FPN_CONV3:
      flags = ip[0];
      ok = flags >= 0 && flags < 4;
      need[0] = pf * 96; need[1] = W33; need[2] = (flags & 1) ? 24 : 0;
      out_rows[0] = pf; out_ld[0] = 24;
      break;
  }
  RT_REQUIRE(ok, s, "rt_debug_fpn: bad parameters for the op");
  RT_REQUIRE(inst, s, "rt_debug_fpn: no kernel instance for this channel split");
  for (int i = 0; i < FPN_IN; i++)
    RT_REQUIRE(need[i] == 0 || (in[i] && in_len[i] >= need[i]), s, "rt_debug_fpn: an operand is missing or too short");
  long long out_n[FPN_OUT];
  for (int i = 0; i < FPN_OUT; i++) {
    out_n[i] = out_ld[i] ? (out_rows[i] + (op == FPN_TAIL ? 1024 : 64)) * out_ld[i] : 0;   // (the map: 64 spare 4 x 4 blocks)
    RT_REQUIRE(out_n[i] == 0 || (out[i] && out_len[i] == out_n[i]), s, "rt_debug_fpn: an output is missing or has the wrong length");
  }
  RT_REQUIRE(s, s, "rt_debug_fpn: null session");
  return guarded(s, [&] {
    RT_HIP_CHECK(hipSetDevice(s->device));
    DevBufs bufs;
    WeightStore ws;
    hipStream_t st = s->st;
    const ImgGeom* dg[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int l = 0; l < n_levels; l++) dg[l] = lv[l].upload(bufs);
    float* dout[FPN_OUT] = {nullptr, nullptr, nullptr};
    for (int i = 0; i < FPN_OUT; i++)
      if (out_n[i]) dout[i] = bufs.canary<float>((size_t)out_n[i], st);
    const bool in_place = op == FPN_UPSAMPLE_ADD && ip[0];
    auto raw = [&](int slot) -> const float* { return need[slot] ? upload_as<float>(bufs, in[slot], (size_t)need[slot]) : nullptr; };
    info_out[0] = 0;
    switch (op) {
      case FPN_PHASE: {
        const int cc = ip[1];
        const bool head = cin == 24;
        nn::FpnPhaseArgs a;
        a.fine = raw(0); a.ld_fine = cf; a.coarse = raw(1); a.ld_coarse = cc;
        if (head) {   // as DetNet's head conv: w = [p5 | p4 | p3 | p2], the fine level is p2, the coarse one p3
          a.Wf = ws.upload(fpn_fine_weights(in[2], 96, 72, 24, 24)); a.wf_img = 0;
          a.Wc = ws.upload(fpn_phase_weights(in[2], 96, 48, 24));
        } else {
          a.Wc = ws.upload(fpn_phase_weights(in[2], 96, 0, 96)); a.wf_img = (long long)216 * cf;
          if (flags & 64) {
            const float* lat = ws.upload(fpn_lateral_weights(in[5], cin, 96));
            const float* wm = ws.upload(fpn_tap_weights(in[2], 96));
            nn::fpn_compose(st, lat, cin, 96, raw(6), wm, cf, n_img, dout[2]);
            a.Wf = dout[2];
          } else {
            a.Wf = raw(4);
          }
        }
        a.fine_scale = raw(7); a.ld_fs = 24; a.coarse_scale = raw(8); a.ld_cs = 24;
        if (flags & 8) { a.G = raw(9); a.gg = dg[2]; a.g_plane = lv[2].total; }
        a.bias = raw(3); a.y = dout[0]; a.ldy = 24;
        if (flags & 2) { a.pool = dout[1]; a.pool_tiles = tiles; }
        a.act = (flags & 4) ? ACT_RELU : ACT_NONE;
        info_out[0] = nn::fpn_phase_instance(cin, cc, a.G != nullptr);
        nn::fpn_phase(st, a, cin, cc, dg[0], dg[1], n_img, maxH, maxW);
      } break;
      case FPN_CLASS: {
        const float* wcls = ws.upload(fpn_class_weights(in[1], 96, ip[0]));
        const float* z = raw(0); const float* bias = raw(2); const float* scale = raw(3); const float* lower = raw(4);
        nn::fpn_class(st, z, 24, scale, 24, dg[0], n_img, lv[0].max_pix, wcls, bias, lower, lower ? dg[1] : nullptr, lower ? pc : 0, dout[0], pf);
      } break;
      case FPN_COMPOSE: {
        const float* lat = ws.upload(fpn_lateral_weights(in[0], cin, 96));
        const float* wm = ws.upload(fpn_tap_weights(in[2], 96));
        nn::fpn_compose(st, lat, cin, 96, raw(1), wm, cf, n_img, dout[0]);
      } break;
      case FPN_TAIL: {
        const ImgGeom* dgo = lv[0].up(4).upload(bufs);
        const float* x = raw(0); const float* w1 = raw(1); const float* b1 = raw(2); const float* w2 = raw(3); const float* b2 = raw(4);
        nn::db_head_tail(st, x, dg[0], dgo, n_img, lv[0].max_pix, w1, b1, w2, b2, dout[0]);
      } break;
      case FPN_LATERAL_ADD: {
        const float* lat = ws.upload(fpn_lateral_weights(in[1], cin, 96));
        const float* x = raw(0); const float* scale = raw(2); const float* b = raw(3);
        nn::lateral_add(st, x, cin, cf, lat, 96, scale, b, dg[0], b ? dg[1] : dg[0], n_img, lv[0].max_pix, dout[0]);
      } break;
      case FPN_UPSAMPLE_ADD: {
        const float* a = nullptr;
        if (in_place) { DevBufs::put(dout[0], in[0], (size_t)need[0]); a = dout[0]; }
        else a = raw(0);
        const float* b = raw(1); const float* scale = raw(2);
        nn::upsample_add(st, a, b, dg[0], dg[1], n_img, lv[0].max_pix, 96, dout[0], scale);
      } break;
      case FPN_SE_PROJECTED: {
        const float* lat = ws.upload(fpn_lateral_weights(in[1], cin, 96));
        float* partial = bufs.alloc<float>((size_t)n_img * nn::pool_chunks(lv[0].max_pix) * cf);
        const float* x = raw(0); const float* w1 = raw(2); const float* b1 = raw(3); const float* w2 = raw(4); const float* b2 = raw(5);
        nn::se_scale_projected(st, x, dg[0], n_img, lv[0].max_pix, cin, cf, lat, 96, 96, w1, b1, w2, b2, ip[1], fp[0], ip[2], partial, dout[0]);
      } break;
      case FPN_SE_TILES: {
        const float* pool = raw(0); const float* w1 = raw(1); const float* b1 = raw(2); const float* w2 = raw(3); const float* b2 = raw(4);
        nn::se_fc_from_tiles(st, pool, dg[0], n_img, tiles, 24, 24, w1, b1, w2, b2, ip[0], fp[0], ip[1], dout[0]);
      } break;
      case FPN_HEAD_FUSED: {
        const PackedDense pw = pack_conv(ws, in[4], (flags & 16) ? in[5] : nullptr, 24, 96, 3, 3);
        const float* p[4]; const float* sc[4];
        for (int l = 0; l < 4; l++) { p[l] = raw(l); sc[l] = raw(6 + l); }
        nn::conv3_fpn_fused(st, p[0], p[1], p[2], p[3], dg[3], dg[2], dg[1], dg[0], n_img, maxH, maxW, 24, sc, pw.w, 24, pw.Npad, dout[0], 24,
                            make_epi(pw, (flags & 32) ? ACT_RELU : ACT_NONE));
      } break;
      case FPN_CONV3: {
        const PackedDense pw = pack_conv(ws, in[1], (flags & 1) ? in[2] : nullptr, 24, 96, 3, 3);
        const Epilogue e = make_epi(pw, (flags & 2) ? ACT_RELU : ACT_NONE);
        info_out[0] = nn::conv_sp_few_groups(3, 3, 24, 24, e);
        nn::conv_sp(st, 3, 3, raw(0), 96, dg[0], n_img, maxH, maxW, 96, pw.w, 24, pw.Npad, dout[0], 24, e);
      } break;
    }
    RT_HIP_CHECK(hipStreamSynchronize(st));
    for (int i = 0; i < FPN_OUT; i++)
      if (out_n[i]) DevBufs::download(out[i], dout[i], (size_t)out_n[i]);
  });
}

// One nh::conv16 launch as the fp16 networks issue it, on host arrays, for tests/test_gpu_f16_kernels.py: a ragged image list
// (or its flat view, one image of 1 x total pixels, as conv_pw16 launches the 1x1 layers), the input as the channel window
// [xoff, xoff + cin) of rows of pitch ldx, the output at (ldy, coff) of a canary-filled buffer with 64 spare rows -- the same
// buffer as the input when in_place, as run_hg_block reads and writes one concat -- and the whole epilogue: bias, activation,
// LAB, a residual with its own pitch, or the dot epilogue of the PFHeadLocal phase convs, which updates the fp32 map `out` holds
// on entry.  route_out receives the nh::Conv16Route of the launch.  Like rt_debug_glue16 it looks at its session last.
//   ip[20]: cin, ldx, xoff, cout, ldy, coff, kh, kw, sh, sw, pt, pl (-1 = k / 2), flat, act, has_lab, ld_res, res_off, in_place,
//           dot_py, dot_px;  fp[3]: lab_a, lab_c, dot_b;  wt [cout][cin][kh][kw];  bias [cout] or NULL;  dot_w [cout] or NULL
RT_API int rt_debug_conv16x(rt_session* s, const int* ip, const float* fp, const int* heights, const int* widths, int n_img,
                            const float* x, long long x_len, const float* wt, long long wt_len, const float* bias, const float* res,
                            long long res_len, const float* dot_w, float* out, long long out_len, int* route_out) {
  RT_REQUIRE(ip && fp && heights && widths && x && wt && out && route_out, s, "rt_debug_conv16x: null argument");
  RT_REQUIRE(n_img > 0 && n_img <= 4096, s, "rt_debug_conv16x: bad image count");
  const int cin = ip[0], ldx = ip[1], xoff = ip[2], cout = ip[3], ldy = ip[4], coff = ip[5], kh = ip[6], kw = ip[7], sh = ip[8], sw = ip[9];
  const int flat = ip[12], act = ip[13], has_lab = ip[14], ld_res = ip[15], res_off = ip[16], in_place = ip[17], py = ip[18], px = ip[19];
  const bool dot = dot_w != nullptr, k22 = kh == 2 && kw == 2;
  RT_REQUIRE(cin > 0 && cin <= 4096 && cout > 0 && cout <= 4096 && ldx > 0 && ldx <= 8192 && xoff >= 0 && xoff + cin <= ldx, s,
             "rt_debug_conv16x: bad channel counts");
  RT_REQUIRE(cin % 8 == 0 && ldx % 8 == 0 && xoff % 8 == 0, s, "rt_debug_conv16x: input channels, pitch and offset must be multiples of 8");
  const int cop = nh::pitch8(cout), npad = round_up(cout, 32);
  RT_REQUIRE(dot || (ldy > 0 && ldy <= 8192 && coff >= 0 && ldy % 8 == 0 && coff % 8 == 0 && coff + cop <= ldy), s,
             "rt_debug_conv16x: the output window must be 8-aligned and lie within its row");
  // the kernel forms the networks launch: odd kernels with "same" padding and strides 1 / 2, 1x1 over the flat view, and the
  // 2x2 phase convs (stride 1, pads 0 / 1, dot epilogue on the instance that holds all 64 channels)
  const int pt = ip[10] < 0 ? kh / 2 : ip[10], pl = ip[11] < 0 ? kw / 2 : ip[11];
  bool ok = sh >= 1 && sh <= 2 && sw >= 1 && sw <= 2 && act >= ACT_NONE && act <= ACT_SIGMOID && (flat == 0 || flat == 1) &&
            (in_place == 0 || in_place == 1) && (has_lab == 0 || has_lab == 1);
  if (k22) ok = ok && dot && sh == 1 && sw == 1 && pt >= 0 && pt <= 1 && pl >= 0 && pl <= 1 && npad == 64 && cin >= 32 && !flat && (py == 0 || py == 1) && (px == 0 || px == 1);
  else ok = ok && !dot && kh >= 1 && kh <= 9 && kw >= 1 && kw <= 9 && (kh & 1) && (kw & 1) && pt == kh / 2 && pl == kw / 2;
  if (flat) ok = ok && kh == 1 && kw == 1 && sh == 1 && sw == 1;
  RT_REQUIRE(ok, s, "rt_debug_conv16x: no such launch in the fp16 networks");
  for (int i = 0; i < n_img; i++)
    RT_REQUIRE(heights[i] > 0 && widths[i] > 0 && heights[i] < 16384 && widths[i] < 16384, s, "rt_debug_conv16x: empty or oversized image");
  // the output: ceil(h / sh) x ceil(w / sw) (the 2x2 phase convs have stride 1: the input's extents); the map of the dot epilogue: twice that
  Ragged gi(heights, widths, n_img), go = gi.down(sh, sw);
  const Ragged gm = go.up(2);
  const long long pin = gi.total, pout = go.total, pmap = gm.total;
  RT_REQUIRE(pin * ldx < (1ll << 28) && pout * std::max(ldy, 1) < (1ll << 28) && pin < (1ll << 24), s, "rt_debug_conv16x: too large");
  if (flat) { gi = gi.flat(); go = gi; }   // (1x1, stride 1: pout == pin)
  RT_REQUIRE(!in_place || (!dot && ldx == ldy && pin == pout), s, "rt_debug_conv16x: in place needs one pitch and one geometry");
  const long long out_n = dot ? pmap + 64 : (pout + 64) * ldy;
  RT_REQUIRE(x_len >= pin * ldx && wt_len == (long long)cout * cin * kh * kw && out_len == out_n, s,
             "rt_debug_conv16x: x is too short, or wt or out has the wrong length");
  RT_REQUIRE(!res || (!dot && ld_res > 0 && ld_res <= 8192 && ld_res % 8 == 0 && res_off >= 0 && res_off % 8 == 0 && res_off + cop <= ld_res &&
                      res_len >= pout * ld_res), s, "rt_debug_conv16x: the residual is misaligned, leaves its row or is too short");
  RT_REQUIRE(s, s, "rt_debug_conv16x: null session");
  return guarded(s, [&] {
    RT_HIP_CHECK(hipSetDevice(s->device));
    DevBufs bufs;
    hipStream_t st = s->st;
    const ImgGeom *dgi = gi.upload(bufs), *dgo = go.upload(bufs), *dgm = gm.upload(bufs);
    const std::vector<half_t> hw = pack_conv16_weights(wt, cout, cin, kh, kw, cin);
    const half_t* dw = bufs.upload(hw.data(), hw.size());
    std::vector<float> hb(npad, 0.f), hd(npad, 0.f);   // bias and dot weights zero beyond cout
    if (bias) memcpy(hb.data(), bias, (size_t)cout * sizeof(float));
    if (dot) memcpy(hd.data(), dot_w, (size_t)cout * sizeof(float));
    const float *db = upload_as<float>(bufs, hb.data(), hb.size()), *dd = upload_as<float>(bufs, hd.data(), hd.size());
    void* dout = dot ? (void*)bufs.canary<float>((size_t)out_n, st) : (void*)bufs.canary<half_t>((size_t)out_n, st);
    half_t* yh = (half_t*)dout; float* yf = (float*)dout;
    if (in_place) put_as(yh, x, (size_t)(pin * ldx));
    const half_t* xh = in_place ? yh : upload_as<half_t>(bufs, x, (size_t)(pin * ldx));
    if (dot) DevBufs::put(yf, out, (size_t)pmap);
    nh::Epi16 e; e.bias = db; e.act = act; e.has_lab = has_lab;
    if (has_lab) { e.lab_a = fp[0]; e.lab_c = fp[1]; }
    if (res) { e.residual = upload_as<half_t>(bufs, res, (size_t)(pout * ld_res)) + res_off; e.ld_res = ld_res; }
    if (dot) { e.dot_w = dd; e.dot_b = fp[2]; e.dot_map = yf; e.gmap = dgm; e.dot_py = py; e.dot_px = px; }
    nh::g_conv16_route = nh::CONV16_ROUTE_NONE;
    nh::conv16(st, xh + xoff, ldx, dgi, dgo, gi.n(), go.maxH, go.maxW, cin, kh, kw, sh, sw, pt, pl, dw, cout, npad, dot ? nullptr : yh + 0,
               dot ? 8 : ldy, dot ? 0 : coff, e);
    *route_out = nh::g_conv16_route;
    RT_HIP_CHECK(hipStreamSynchronize(st));
    if (dot) DevBufs::download(out, yf, (size_t)out_n); else DevBufs::download(out, yh, (size_t)out_n);
  });
}

// One MobileNetV3 block of the angle classifier through the networks' run_cls_block on host arrays (tests/test_gpu_cls_kernels.py
// compares it with an fp64 block): n crops of one H x W, as ClsNet has them (cls_block_supported() sees the maxima only), the weights
// through the packers ClsNet's constructor calls, squeeze-excite on mid / 4 hidden units, the shortcut where ClsNet takes it
// (stride 1 and cin == cout).  form = nn::g_cls_fused for the launch; what ran is reported, not recomputed: cls_block_fused() and
// cls_block_shape() are what run_cls_block and nn::cls_block themselves ask.  The session is looked at last.
RT_API int rt_debug_cls_block(rt_session* s, const float* x, int n, int H, int W, int cin, int mid, int cout, int k, int sh, int act,
                              int se, const float* exp_w, const float* exp_b, const float* dw_w, const float* dw_b, const float* fc1_w,
                              const float* fc1_b, const float* fc2_w, const float* fc2_b, const float* lin_w, const float* lin_b,
                              int form, float* out, int* info_out) {
  RT_REQUIRE(x && exp_w && exp_b && dw_w && dw_b && lin_w && lin_b && out && info_out, s, "rt_debug_cls_block: null argument");
  RT_REQUIRE((se == 0 || se == 1) && (!se || (fc1_w && fc1_b && fc2_w && fc2_b)), s, "rt_debug_cls_block: a squeeze-excite block needs both FCs");
  RT_REQUIRE(n > 0 && n <= 4096 && H > 0 && H <= 4096 && W > 0 && W <= 4096, s, "rt_debug_cls_block: bad crop count or extents");
  RT_REQUIRE(cin > 0 && cin <= 64 && cin % 4 == 0 && cout > 0 && cout <= 64 && cout % 4 == 0 && mid >= 4 && mid <= 1024 && mid % 4 == 0,
             s, "rt_debug_cls_block: channel counts must be multiples of 4 (cin, cout <= 64, mid <= 1024)");
  RT_REQUIRE((k == 3 || k == 5) && (sh == 1 || sh == 2) && (act == ACT_RELU || act == ACT_HSWISH) && (form == 0 || form == 1), s,
             "rt_debug_cls_block: no such block in the classifier");
  RT_REQUIRE((long long)n * H * W * chan_pitch(mid) < (1ll << 27), s, "rt_debug_cls_block: too large");
  RT_REQUIRE(s, s, "rt_debug_cls_block: null session");
  return guarded(s, [&] {
    s->begin_call();
    WeightStore ws;
    ClsBlock b;
    b.expand = pack_conv(ws, exp_w, exp_b, mid, cin, 1, 1);
    b.dw = pack_dw(ws, dw_w, dw_b, mid, k);
    b.se = se != 0;
    if (se) b.sew = get_se(ws, fc1_w, fc1_b, fc2_w, fc2_b, mid, mid / 4);
    b.linear = pack_conv(ws, lin_w, lin_b, cout, mid, 1, 1);
    b.act = act; b.sh = sh; b.sw = 1; b.cin = cin; b.shortcut = sh == 1 && cin == cout;
    Level Li = make_level(std::vector<std::pair<int, int>>((size_t)n, {H, W})), Lo = down_level(Li, sh, 1);
    DevBufs bufs;
    RestoreInt keep_form(nn::g_cls_fused);
    nn::g_cls_fused = form;
    RunCtx c = s->ctx(&s->arena);
    upload_levels(c, {&Li, &Lo});
    const size_t nin = (size_t)Li.total * cin, nout = (size_t)(Lo.total + 64) * cout;
    float* dx = bufs.zeroed<float>(nin + (size_t)256 * cin);   // (zero rows past the last crop: the series' GEMM tiles read them)
    DevBufs::put(dx, x, nin);
    float* dy = bufs.canary<float>(nout, s->st);
    const bool fused = cls_block_fused(b, Li, Lo);
    run_cls_block(c, b, dx, Li, Lo, dy);
    RT_HIP_CHECK(hipStreamSynchronize(s->st));
    DevBufs::download(out, dy, nout);
    const nn::ClsBlockShape sp = nn::cls_block_shape(k, cin, mid, Li.maxH, Li.maxW, (int)Lo.maxPix);
    info_out[0] = fused ? 1 : 0; info_out[1] = fused && sp.padrow ? 1 : 0; info_out[2] = fused ? sp.maxu : 0; info_out[3] = fused ? sp.lds : 0;
  });
}

// One stem launch (3x3, stride 2, pad 1, 3 -> cout channels) on a ragged image list, as the three networks issue it: cout 8 =
// nn::stem_conv -> k_stem<8> (the classifier's), cout 16 with x4 = nn::stem_conv -> k_stem_mfma<0> (the rec net's), cout 16 with
// rgb = nn::stem_conv_u8 -> k_stem_mfma<1> over U8Page descriptors built on the uploaded pages, as det_groups builds them (the
// det net's; scale / mean3 / std3 = the normalisation folded in).  Weights through pack_stem.  The session is looked at last.
RT_API int rt_debug_stem(rt_session* s, const float* x4, const unsigned char* rgb, const int* heights, const int* widths, int n_img,
                         int cout, const float* w, const float* bias, int act, float scale, const float* mean3, const float* std3,
                         float* out, long long out_len) {
  RT_REQUIRE(heights && widths && w && bias && out && ((x4 != nullptr) != (rgb != nullptr)), s, "rt_debug_stem: null argument (x4 or rgb, not both)");
  RT_REQUIRE(n_img > 0 && n_img <= 4096 && (cout == 16 || (cout == 8 && x4)) && act >= ACT_NONE && act <= ACT_SIGMOID, s,
             "rt_debug_stem: bad image count, activation or cout (8 or 16 from a tensor, 16 from pages)");
  RT_REQUIRE(!rgb || (mean3 && std3 && std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f), s, "rt_debug_stem: pages need mean3 and a non-zero std3");
  for (int i = 0; i < n_img; i++)
    RT_REQUIRE(heights[i] > 0 && widths[i] > 0 && heights[i] <= 4096 && widths[i] <= 4096, s, "rt_debug_stem: empty or oversized image");
  const Ragged gi(heights, widths, n_img), go = gi.down(2, 2);
  RT_REQUIRE(gi.total < (1ll << 24), s, "rt_debug_stem: too large");
  const long long out_n = (go.total + 64) * cout;
  RT_REQUIRE(out_len == out_n, s, "rt_debug_stem: out has the wrong length");
  RT_REQUIRE(s, s, "rt_debug_stem: null session");
  return guarded(s, [&] {
    RT_HIP_CHECK(hipSetDevice(s->device));
    WeightStore ws;
    float *dw = nullptr, *db = nullptr;
    pack_stem(ws, w, bias, cout, &dw, &db);
    DevBufs bufs;
    const ImgGeom *dgi = gi.upload(bufs), *dgo = go.upload(bufs);
    float* dy = bufs.canary<float>((size_t)out_n, s->st);
    if (rgb) {
      const uint8_t* d8 = bufs.upload(rgb, (size_t)gi.total * 3);
      std::vector<nn::U8Page> pages(n_img);
      for (int i = 0; i < n_img; i++) pages[i] = nn::U8Page{d8 + gi.g[i].off * 3, (long long)gi.g[i].H * gi.g[i].W, gi.g[i].off};
      nn::stem_conv_u8(s->st, bufs.upload(pages.data(), pages.size()), scale, mean3, std3, dgi, dgo, n_img, go.maxH, go.maxW, cout, dw, db, act, dy);
    } else {
      nn::stem_conv(s->st, bufs.upload(x4, (size_t)gi.total * 4), dgi, dgo, n_img, go.maxH, go.maxW, cout, dw, db, act, dy);
    }
    RT_HIP_CHECK(hipStreamSynchronize(s->st));
    DevBufs::download(out, dy, (size_t)out_n);
  });
}

// One launch (squeeze-excite: the launch pair, plus nn::scale_channels in place, as run_se issues them) of the fp32 glue around the
// squeeze-excite blocks and the classifier's and rec net's tails, on host arrays, for tests/test_gpu_cls_kernels.py
// (include/retto_hip.h lists the ops).  Every address a kernel can form is checked against the callers' lengths first; the session
// is looked at last.
namespace {
enum Glue32Op { G32_SE_SCALE = 0, G32_GLOBAL_MEAN, G32_MAXPOOL, G32_AVGPOOL, G32_SOFTMAX, G32_ARGMAX_PROB, G32_ARGMAX, G32_COUNT };
}  // namespace
RT_API int rt_debug_glue32(rt_session* s, int op, const int* ip, const float* fp, const int* heights, const int* widths, int n_img,
                           const float* x, long long x_len, const float* const* w, float* out, long long out_len, float* out2,
                           long long out2_len, int* idx_out) {
  RT_REQUIRE(ip && fp && x && out, s, "rt_debug_glue32: null argument");
  RT_REQUIRE(op >= 0 && op < G32_COUNT && n_img > 0 && n_img <= 4096, s, "rt_debug_glue32: bad op or image / row count");
  const bool rows_op = op >= G32_SOFTMAX;   // n_img = the rows; no geometry
  RT_REQUIRE(rows_op || (heights && widths), s, "rt_debug_glue32: null geometry");
  for (int i = 0; !rows_op && i < n_img; i++)
    RT_REQUIRE(heights[i] > 0 && widths[i] > 0 && heights[i] <= 4096 && widths[i] <= 4096, s, "rt_debug_glue32: empty or oversized image");
  const Ragged gi = rows_op ? Ragged() : Ragged(heights, widths, n_img);
  Ragged go;
  const int C = ip[0];
  RT_REQUIRE(C > 0 && C <= 8192, s, "rt_debug_glue32: bad channel count");
  int Cp = C, ldy = C, Cr = 0;
  long long x_need = 0, out_rows = 0, out2_n = 0;
  bool ok = true;
  switch (op) {
    case G32_SE_SCALE:   // ip = {C, Cr, residual, apply}; fp = {slope}
      Cp = chan_pitch(C); Cr = ip[1]; ldy = Cp;
      ok = C % 4 == 0 && Cr > 0 && Cr <= 1024 && (ip[2] == 0 || ip[2] == 1) && (ip[3] == 0 || ip[3] == 1) && fp[0] > 0.f && fp[0] <= 1.f &&
           w && w[0] && w[1] && w[2] && w[3];
      x_need = gi.total * Cp; out_rows = n_img; out2_n = ip[3] ? (gi.total + 64) * Cp : 0;
      break;
    case G32_GLOBAL_MEAN: ok = C % 4 == 0; x_need = gi.total * Cp; out_rows = n_img; break;
    case G32_MAXPOOL:
      ok = C % 4 == 0;
      for (int i = 0; ok && i < n_img; i++) ok = heights[i] >= 2 && widths[i] >= 2;
      if (ok) go = gi.pool(2, 2);
      x_need = gi.total * Cp; out_rows = go.total;
      break;
    case G32_AVGPOOL:    // ip = {Cp, ldy}
      ldy = ip[1];
      ok = C % 4 == 0 && ldy >= C && ldy <= 16384 && ldy % 4 == 0;
      for (int i = 0; ok && i < n_img; i++) ok = heights[i] >= 3 && widths[i] >= 2;
      if (ok) go = gi.pool(3, 2);
      x_need = gi.total * Cp; out_rows = go.total;
      break;
    case G32_SOFTMAX: case G32_ARGMAX_PROB: case G32_ARGMAX:   // ip = {C, ld}
      ok = ip[1] >= C && ip[1] <= 16384 && (op == G32_SOFTMAX || idx_out);
      x_need = (long long)n_img * ip[1]; out_rows = n_img; ldy = op == G32_SOFTMAX ? C : 1;
      break;
  }
  RT_REQUIRE(ok, s, "rt_debug_glue32: bad parameters for the op");
  RT_REQUIRE(x_need < (1ll << 28) && out_rows * ldy < (1ll << 28), s, "rt_debug_glue32: too large");
  const long long out_n = (out_rows + 64) * ldy;
  RT_REQUIRE(x_len >= x_need && out_len == out_n, s, "rt_debug_glue32: x is too short or out has the wrong length");
  RT_REQUIRE(out2_n == 0 || (out2 && out2_len == out2_n), s, "rt_debug_glue32: out2 is missing or has the wrong length");
  RT_REQUIRE(s, s, "rt_debug_glue32: null session");
  return guarded(s, [&] {
    RT_HIP_CHECK(hipSetDevice(s->device));
    DevBufs bufs;
    WeightStore ws;
    hipStream_t st = s->st;
    float* dout = bufs.canary<float>((size_t)out_n, st);
    const ImgGeom* dgi = rows_op ? nullptr : gi.upload(bufs);
    switch (op) {
      case G32_SE_SCALE: {   // as run_se
        const SeW se = get_se(ws, w[0], w[1], w[2], w[3], C, Cr);
        float* dx = nullptr;
        if (out2_n) { dx = bufs.canary<float>((size_t)out2_n, st); DevBufs::put(dx, x, (size_t)x_need); }
        else dx = bufs.upload(x, (size_t)x_need);
        float* partial = bufs.alloc<float>((size_t)n_img * nn::pool_chunks(gi.max_pix) * Cp);
        nn::se_scale(st, dx, dgi, n_img, gi.max_pix, se.C, Cp, se.w1, se.b1, se.w2, se.b2, se.Cr, fp[0], ip[2], partial, dout);
        if (out2_n) nn::scale_channels(st, dx, dgi, n_img, gi.max_pix, Cp, dout);
        RT_HIP_CHECK(hipStreamSynchronize(st));
        if (out2_n) DevBufs::download(out2, dx, (size_t)out2_n);
      } break;
      case G32_GLOBAL_MEAN: {
        float* partial = bufs.alloc<float>((size_t)n_img * nn::pool_chunks(gi.max_pix) * Cp);
        nn::global_mean(st, bufs.upload(x, (size_t)x_need), dgi, n_img, gi.max_pix, Cp, partial, dout);
      } break;
      case G32_MAXPOOL: nn::maxpool_2x2(st, bufs.upload(x, (size_t)x_need), dgi, go.upload(bufs), n_img, go.max_pix, Cp, dout); break;
      case G32_AVGPOOL: nn::avgpool_3x2(st, bufs.upload(x, (size_t)x_need), dgi, go.upload(bufs), n_img, go.max_pix, Cp, dout, ldy); break;
      case G32_SOFTMAX: nn::softmax_rows(st, bufs.upload(x, (size_t)x_need), ip[1], n_img, C, dout); break;
      case G32_ARGMAX_PROB: case G32_ARGMAX: {
        int* didx = bufs.canary<int>((size_t)out_n, st);
        const float* dx = bufs.upload(x, (size_t)x_need);
        if (op == G32_ARGMAX_PROB) nn::argmax_prob_rows(st, dx, ip[1], n_img, C, didx, dout);
        else nn::argmax_rows(st, dx, ip[1], n_img, C, didx, dout);
        RT_HIP_CHECK(hipStreamSynchronize(st));
        DevBufs::download(idx_out, didx, (size_t)out_n);
      } break;
    }
    RT_HIP_CHECK(hipStreamSynchronize(st));
    DevBufs::download(out, dout, (size_t)out_n);
  });
}

// Kernel micro-benchmark: one LCNetV3 block (3x3 depthwise -> pointwise) through the networks' run_lc on n images of h x w pixels,
// random data.  form = nn::g_lc_wave for the timed launches: 0 = k_lc_thin (workgroup-staged; the unfused depthwise + GEMM pair where
// it has no instance), 1 = k_lc_wave (direct loads, stride 1), 3 = k_lc_lds (production); stride 21 means (2, 1).  maxdiff compares
// with form 0.
RT_API int rt_bench_lc(rt_session* s, int n, int h, int w, int cin, int cout, int stride, int form, int iters, float* ms_out, float* maxdiff_out) {
  RT_REQUIRE(s && ms_out && n > 0 && h > 0 && w > 0 && cin > 0 && cout > 0 && (stride == 1 || stride == 2 || stride == 21), s, "rt_bench_lc: bad argument");
  return guarded(s, [&] {
    s->begin_call();
    const int sh = stride == 21 ? 2 : stride, sw = stride == 21 ? 1 : stride;   // 21: stride (2, 1)
    std::vector<float> hwd((size_t)cin * 9), hbd(cin), hw((size_t)cout * cin), hb(cout);
    uint32_t st = 777;
    auto rnd = [&]() { st = st * 1664525u + 1013904223u; return ((st >> 8) & 0xffff) / 32768.0f - 1.0f; };
    for (auto& v : hwd) v = rnd() * 0.3f;
    for (auto& v : hw) v = rnd() * 0.1f;
    for (auto& v : hbd) v = rnd() * 0.1f;    // (a bias per channel: a constant one would hide an indexing error)
    for (auto& v : hb) v = rnd() * 0.2f;
    const bool plain_tail = sh == 2 && sw == 2;   // (depthwise tail as in the LCNetV3 blocks)
    WeightStore ws;
    const LcBlock blk = debug_lc_block(ws, cin, cout, sh, sw, hwd.data(), hbd.data(), hw.data(), hb.data(), plain_tail ? ACT_NONE : ACT_HSWISH,
                                     Lab{!plain_tail, 0.99f, 0.01f}, Lab{1, 1.01f, 0.02f});
    Level Li = make_level(std::vector<std::pair<int, int>>((size_t)n, {h, w})), Lo = down_level(Li, sh, sw);
    RunCtx c = s->ctx(&s->arena);
    upload_levels(c, {&Li, &Lo});
    const size_t nin = (size_t)Li.total * blk.dw.Cp, nout = (size_t)Lo.total * chan_pitch(cout);
    std::vector<float> hx(nin, 0.f);
    for (size_t p = 0; p < (size_t)Li.total; p++) for (int k = 0; k < cin; k++) hx[p * blk.dw.Cp + k] = rnd();
    DevBufs bufs;
    RestoreInt keep_form(nn::g_lc_wave);
    float *dx = bufs.upload(hx.data(), nin), *dy = bufs.zeroed<float>(nout), *dy0 = bufs.zeroed<float>(nout);
    float* dy1 = nullptr;   // depthwise output of the unfused route
    auto run = [&](float* out) {
      if (!dy1) dy1 = debug_lc_mid(bufs, s->st, blk, Lo);
      run_lc(c, blk, dx, Li, Lo, out, dy1);
    };
    nn::g_lc_wave = 0; run(dy0);
    nn::g_lc_wave = form;
    timed_and_compared(s->st, iters, [&] { run(dy); }, dy0, dy, nout, ms_out, maxdiff_out);
  });
}

// The det stage of a one-page pipeline call on a host RGB8 image at det-input size, under the session's det tiles: det_groups itself
// (rt_session::debug_det_tiles), for tests/test_gpu_det_tiles.py.
RT_API int rt_debug_det_tiles(rt_session* s, const uint8_t* rgb_det, int h, int w, float* tile_maps_out, float* page_map_out) {
  RT_REQUIRE(s && rgb_det && page_map_out, s, "rt_debug_det_tiles: null argument");
  return guarded(s, [&] { s->debug_det_tiles(rgb_det, h, w, tile_maps_out, page_map_out); });
}
// n lines of [3, 48, widths[i]] as ONE rec group through the pipeline's own cut, network and stitch, under the session's rec
// windows (rt_session::debug_rec_windows), for tests/test_gpu_rec_windows.py.
RT_API int rt_debug_rec_windows(rt_session* s, const float* nchw, int n, const int* widths, int32_t* unit_idx_out, float* unit_prob_out,
                                float* unit_z5_out, int32_t* line_idx_out, float* line_prob_out, float* line_z5_out) {
  RT_REQUIRE(s && nchw && widths && n > 0, s, "rt_debug_rec_windows: bad argument");
  return guarded(s, [&] {
    s->debug_rec_windows(nchw, n, widths, unit_idx_out, unit_prob_out, unit_z5_out, line_idx_out, line_prob_out, line_z5_out);
  });
}
// n RGB8 crops as ONE rec group through the pipeline's own rotate, resize_norm, network, score and select, under the session's rec
// windows (rt_session::debug_rec_flip), for tests/test_gpu_rec_flip.py.  Everything is checked before any device work.
RT_API int rt_debug_rec_flip(rt_session* s, const uint8_t* crops, const int32_t* hw, int n, const uint8_t* both, float max_wh_ratio,
                             int32_t* view_idx_out, float* view_prob_out, float* view_z5_out, int32_t* view_ntok_out,
                             float* view_score_out, int32_t* taken_out, int32_t* idx_out, float* prob_out, float* z5_out) {
  RT_REQUIRE(s && crops && hw && both && n > 0, s, "rt_debug_rec_flip: bad argument");
  RT_REQUIRE(max_wh_ratio > 0.0f && max_wh_ratio - max_wh_ratio == 0.0f && max_wh_ratio <= 1024.0f, s,
             "rt_debug_rec_flip: max_wh_ratio must be positive, finite and at most 1024");
  for (int i = 0; i < n; i++)
    RT_REQUIRE(hw[2 * i] >= 1 && hw[2 * i + 1] >= 1 && hw[2 * i] <= 16384 && hw[2 * i + 1] <= 16384, s,
               "rt_debug_rec_flip: every crop must be 1 .. 16384 pixels either way");
  return guarded(s, [&] {
    rt_session::RecFlipOut out;
    out.view_idx = view_idx_out; out.view_prob = view_prob_out; out.view_z5 = view_z5_out; out.view_ntok = view_ntok_out; out.view_score = view_score_out;
    out.taken = taken_out; out.idx = idx_out; out.prob = prob_out; out.z5 = z5_out;
    s->debug_rec_flip(crops, hw, n, both, max_wh_ratio, out);
  });
}
// The main lane's arenas, for tools/bench_det_tiles.py: the largest pass so far of the call arena, the scratch arena (network
// activations, rewound per launch group) and the DB post-processing workspace, in bytes.
RT_API int rt_debug_arena_high_water(rt_session* s, long long* out3) {
  RT_REQUIRE(s && out3, s, "rt_debug_arena_high_water: null argument");
  return guarded(s, [&] {
    out3[0] = (long long)s->arena.high_water(); out3[1] = (long long)s->scratch.high_water(); out3[2] = (long long)s->dbws.high_water();
  });
}
// iters device-to-device hipMemcpyAsync of `bytes` bytes on the session's stream between two buffers of their own, timed with
// events: *ms_out = the mean per copy.  The yardstick tools/bench_det_tiles.py states the cut and stitch kernels against.
RT_API int rt_bench_memcpy_d2d(rt_session* s, size_t bytes, int iters, float* ms_out) {
  RT_REQUIRE(s && ms_out && bytes > 0 && iters > 0, s, "rt_bench_memcpy_d2d: bad argument");
  return guarded(s, [&] {
    RT_HIP_CHECK(hipSetDevice(s->device));
    DevBufs bufs;
    char* a = bufs.zeroed<char>(bytes); char* b = bufs.zeroed<char>(bytes);
    Events ev;
    RT_HIP_CHECK(hipEventCreate(&ev.a)); RT_HIP_CHECK(hipEventCreate(&ev.b));
    RT_HIP_CHECK(hipMemcpyAsync(b, a, bytes, hipMemcpyDeviceToDevice, s->st));   // (warm-up)
    RT_HIP_CHECK(hipEventRecord(ev.a, s->st));
    for (int i = 0; i < iters; i++) RT_HIP_CHECK(hipMemcpyAsync(b, a, bytes, hipMemcpyDeviceToDevice, s->st));
    RT_HIP_CHECK(hipEventRecord(ev.b, s->st));
    RT_HIP_CHECK(hipStreamSynchronize(s->st));
    float ms = 0.f;
    RT_HIP_CHECK(hipEventElapsedTime(&ms, ev.a, ev.b));
    *ms_out = ms / (float)iters;
  });
}

}  // extern "C"
