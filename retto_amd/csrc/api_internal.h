// What the extern "C" entry points of api.cpp (the library's surface), api_ctc.cpp (the rec CTC tail's debug entries) and
// api_debug.cpp (the kernel diagnostics) share: the exception guard with the drain of every lane's stream, the argument-check
// macro, and the RAII pieces and ragged layout of the diagnostic hooks.  The hooks take the session where they mean lane 0
// (rt_session is an rt_lane).  Internal: nothing here is exported.
#pragma once
#include <algorithm>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "session.h"

namespace rt {

std::string& create_error();       // the calling thread's message for calls without a session: what rt_last_error(NULL) returns
void capture_variant_defaults();   // the A/B switches' load-time values (rt_debug_set_variants restores to them)

// A call that fails after work was enqueued must not leave kernels or H2D copies in flight: the next
// begin_call() rewinds the pinned staging and the arenas they read.  Errors of the drain itself are dropped
// (the first failure is the one reported).
inline void quiesce(rt_session* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  for (int l = 0; l < s->n_lanes(); l++)
    if (s->lane(l)->st) (void)hipStreamSynchronize(s->lane(l)->st);
  (void)hipGetLastError();
}
// ALLOW_INFLIGHT: only rt_submit_batch / rt_wait_batch may run while submitted batches are in flight -- every other entry point
// uses the main lane's stream and arenas, which lane 0's worker thread owns until the last ticket has been waited for.
template <bool ALLOW_INFLIGHT = false, typename F>
int guarded(rt_session* s, F&& f) {
  if (!ALLOW_INFLIGHT && s && s->inflight.load() > 0) {
    s->last_error = "batches submitted with rt_submit_batch are in flight: call rt_wait_batch for every ticket first";
    return RT_ERR_INVALID;
  }
  // rt_session::last_error is written and cleared on the API caller's thread only (here, RT_REQUIRE, the shape checks): lane
  // threads keep their failure in the ticket (rt_ticket::errs) and it surfaces through rt_wait_batch's rethrow below.
  // On the ALLOW_INFLIGHT path nothing is drained here: the lane that failed has drained its own stream in the worker, and the
  // streams of the other lanes carry OTHER batches that a failed ticket must not stall.
  if (s) s->last_error.clear();
  try {
    f();
    return RT_OK;
  } catch (const RtError& e) {
    if (!ALLOW_INFLIGHT) quiesce(s);
    (s ? s->last_error : create_error()) = e.what();
    return e.code;
  } catch (const std::bad_alloc&) {
    if (!ALLOW_INFLIGHT) quiesce(s);
    (s ? s->last_error : create_error()) = "out of host memory";
    return RT_ERR_BACKEND;
  } catch (const std::exception& e) {
    if (!ALLOW_INFLIGHT) quiesce(s);
    (s ? s->last_error : create_error()) = e.what();
    return RT_ERR_BACKEND;
  }
}
#define RT_REQUIRE(cond, s, msg)                                             \
  do {                                                                        \
    if (!(cond)) {                                                            \
      if (s) (s)->last_error = msg; else rt::create_error() = msg;            \
      return RT_ERR_INVALID;                                                  \
    }                                                                         \
  } while (0)

// RAII for the diagnostic hooks: a process-wide A/B switch is put back and the scratch buffers are freed on EVERY way out of
// the hook (an RT_HIP_CHECK that throws used to leave the switch at the benchmark's value for every later call).
struct RestoreInt { int& ref; int old; explicit RestoreInt(int& r) : ref(r), old(r) {} ~RestoreInt() { ref = old; } };
struct ForgetSplit { const float* w; ~ForgetSplit() { nn::gemm_split_forget(w); } };
struct Events { hipEvent_t a = nullptr, b = nullptr; ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } };
// Device scratch of one hook.  Every copy is a blocking hipMemcpy, which is NOT ordered with the session's (non-blocking)
// stream: an entry synchronises the stream between its launches and download(), and canary() does so after its fill.
struct DevBufs {
  std::vector<void*> p;
  ~DevBufs() { for (void* q : p) (void)hipFree(q); }
  template <typename T> T* alloc(size_t n) { void* q = nullptr; RT_HIP_CHECK(hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T))); p.push_back(q); return (T*)q; }
  template <typename T> T* zeroed(size_t n) { T* d = alloc<T>(n); RT_HIP_CHECK(hipMemset(d, 0, n * sizeof(T))); return d; }
  template <typename T> static void put(T* dev, const T* host, size_t n) { RT_HIP_CHECK(hipMemcpy(dev, host, n * sizeof(T), hipMemcpyHostToDevice)); }
  template <typename T> T* upload(const T* host, size_t n) { T* d = alloc<T>(n); put(d, host, n); return d; }
  // n elements of RT_DEBUG_CANARY words.  Halves are filled two a word, so an odd n takes one half more (the kernels under
  // test never see it).  The stream is drained before returning: a blocking copy into the buffer (an operand that is also the
  // output) then lands after the fill, whichever entry makes it.
  template <typename T> T* canary(size_t n, hipStream_t st) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 2, "a canary word is one float or two halves");
    T* d = alloc<T>(sizeof(T) == 2 ? n + 1 : n);
    RT_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)d, (int)RT_DEBUG_CANARY, sizeof(T) == 2 ? (n + 1) / 2 : n, st));
    RT_HIP_CHECK(hipStreamSynchronize(st));
    return d;
  }
  // n elements back to the host, converted where the types differ (halves to float)
  template <typename H, typename T> static void download(H* host, const T* dev, size_t n) {
    if constexpr (std::is_same<H, T>::value) {
      RT_HIP_CHECK(hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost));
    } else {
      std::vector<T> h(n);
      RT_HIP_CHECK(hipMemcpy(h.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost));
      for (size_t i = 0; i < n; i++) host[i] = (H)h[i];
    }
  }
};
// a host float array on the device as T (the debug entries take float32 and convert): into a buffer there is, or a new one
template <typename T> void put_as(T* dev, const float* src, size_t n) {
  std::vector<T> h(std::max<size_t>(n, 1));
  for (size_t i = 0; i < n; i++) h[i] = (T)src[i];
  DevBufs::put(dev, h.data(), n);
}
template <typename T> T* upload_as(DevBufs& bufs, const float* src, size_t n) { T* d = bufs.alloc<T>(n); put_as(d, src, n); return d; }

// A ragged list of images laid out back to back, as the networks' levels are: each image's offset in pixels, the total, the
// largest extents.  It accumulates; what an entry accepts (empty, oversized) is the entry's own check, made before.
struct Ragged {
  std::vector<ImgGeom> g;
  long long total = 0, max_pix = 0;
  int maxH = 0, maxW = 0;
  Ragged() = default;
  Ragged(const int* hs, const int* ws, int n) { for (int i = 0; i < n; i++) push(hs[i], ws[i]); }
  // token lines (or image row counts): one ImgGeom{off, 1, T} each, as SvtrCore passes its token level
  template <typename I> Ragged(const I* tokens, int n) { for (int i = 0; i < n; i++) push(1, (int)tokens[i]); }
  void push(int h, int w) {
    g.push_back(ImgGeom{total, h, w, 0});
    const long long pix = (long long)h * w;
    total += pix; max_pix = std::max(max_pix, pix); maxH = std::max(maxH, h); maxW = std::max(maxW, w);
  }
  int n() const { return (int)g.size(); }
  Ragged down(int sh, int sw) const { Ragged r; for (const ImgGeom& i : g) r.push((i.H + sh - 1) / sh, (i.W + sw - 1) / sw); return r; }   // a "same"-padded conv of stride (sh, sw)
  Ragged up(int k) const { Ragged r; for (const ImgGeom& i : g) r.push(k * i.H, k * i.W); return r; }
  Ragged pool(int kh, int kw) const { Ragged r; for (const ImgGeom& i : g) r.push(i.H / kh, i.W / kw); return r; }   // window = stride, no padding (pool_level)
  Ragged flat() const { Ragged r; r.push(1, (int)total); return r; }   // one image of 1 x total pixels
  const ImgGeom* upload(DevBufs& bufs) const { return bufs.upload(g.data(), g.size()); }
};

}  // namespace rt
