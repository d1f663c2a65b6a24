// What the extern "C" entry points of api.cpp (the library's surface) and api_debug.cpp (the kernel diagnostics) share: the
// exception guard, the argument-check macro, and the RAII pieces of the diagnostic hooks.  Internal: nothing here is exported.
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
// what both rt_debug_ctc_candidates forms require of their arguments; *rows_out = the lines' time steps
bool cand_args_ok(const float* z5, const float* W, int N, const int32_t* idx, const float* prob, const int32_t* tokens_per_line,
                  int n_lines, int K, const rt_candidate* cands_out, const int32_t* cols_out, const int32_t* n_tokens_out,
                  long long* rows_out);

// what both rt_debug_ctc_charset forms require beyond cand_args_ok (K = 0 allowed there: cands / cols may then be NULL)
bool charset_args_ok(const float* z5, const float* W, int N, const int32_t* idx, const float* prob, const int32_t* tokens_per_line,
                     int n_lines, const int32_t* line_set, const uint32_t* masks, int n_sets, int K, const int32_t* tokens_out,
                     const int32_t* n_tokens_out, const float* scores_out, const rt_candidate* cands_out, const int32_t* cols_out,
                     long long* rows_out);

// what both rt_debug_ctc_lexicon forms require of their arguments: the first requirement that fails, in words, or the empty
// string; *rows_out = the lines' time steps, *table_out = the floats of the loglik table (one per entry of the lexicon of every
// line that has one)
std::string lexicon_args_error(const float* z5, const float* W, int N, const int32_t* tokens_per_line, int n_lines,
                               const int32_t* line_lex, const int32_t* entry_ids, const int32_t* entry_lens,
                               const int32_t* lex_first_entry, int n_lex, const rt_lexicon_match* matches_out,
                               const int32_t* n_matches_out, long long* rows_out, long long* table_out);
// what both rt_debug_ctc_keywords forms require of their arguments, likewise; *table_out = the entries of the score / span tables
std::string keywords_args_error(const float* z5, const float* W, int N, const int32_t* tokens_per_line, int n_lines,
                                const int32_t* line_kw, const int32_t* entry_ids, const int32_t* entry_lens,
                                const int32_t* kw_first_entry, int n_kw, const float* kw_min_score, const rt_keyword_hit* hits_out,
                                const int32_t* n_hits_out, long long* rows_out, long long* table_out);
// what both rt_debug_ctc_beam forms require of their arguments, likewise (beam = 0, off, and n_lines = 0 pass: the entries then
// do nothing); *rows_out = the lines' time steps
std::string beam_args_error(const float* z5, const float* W, int N, const int32_t* tokens_per_line, int n_lines, int beam, int nbest,
                            const int32_t* counts_out, const rt_beam* beams_out, const int32_t* tokens_out, long long* rows_out);
// what both rt_debug_ctc_lexicon_align forms require beyond lexicon_args_error (n_lex already checked), likewise
std::string lexicon_align_args_error(const float* lex_min_post, int n_lex, const int32_t* idx, const float* prob,
                                     const int32_t* snapped_out, const float* vit_out);
// what both rt_debug_ctc_pattern forms require of their arguments, likewise; rules_out: the n_pat patterns' tables (pt::Rule::build
// checks the flat compiled tables: pattern k's group_of at [k][N], its delta [S[k]][G[k]] and accept [S[k]] behind pattern k - 1's)
std::string pattern_args_error(const float* z5, const float* W, int N, const int32_t* tokens_per_line, int n_lines,
                               const int32_t* line_pat, const int32_t* pat_S, const int32_t* pat_G, const int32_t* group_of,
                               const int32_t* delta, const int32_t* accept, int n_pat, const int32_t* idx, const float* prob,
                               const int32_t* matched_out, const float* vit_out, const float* logprob_out, const float* free_out,
                               long long* rows_out, std::vector<pt::Rule>* rules_out);

// A call that fails after work was enqueued must not leave kernels or H2D copies in flight: the next
// begin_call() rewinds the pinned staging and the arenas they read.  Errors of the drain itself are dropped
// (the first failure is the one reported).
inline void quiesce(rt_session* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  if (s->st) (void)hipStreamSynchronize(s->st);
  for (auto& h : s->helpers)
    if (h->st) (void)hipStreamSynchronize(h->st);
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

}  // namespace rt
