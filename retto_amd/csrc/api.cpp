// extern "C" surface of libretto_hip.so (include/retto_hip.h): sessions, the networks, the pipeline stages, batches, results,
// parsers and device memory, with the four feature-level debug hooks that are thin forwards into their features
// (rt_debug_warp_crops, rt_debug_jpeg_reconstruct, rt_debug_word_boxes, rt_debug_span_quad).  The debug entries of the rec CTC
// tail's options (rt_debug_ctc_*, both forms, and rt_debug_*_compile) are in api_ctc.cpp, on the host references of
// ctc_host_ref.h; it also asserts the layouts the rt_results_rec_* accessors here cast between.  The kernel-level diagnostics
// (rt_debug_set_variants, rt_bench_*, and the rt_debug_* harnesses the kernel tests drive) are in api_debug.cpp; api_internal.h
// holds what the three share.  A pipeline entry checks its arguments, makes the call a PageCall (rt_session::call_of) and hands it
// to the session; rt_destroy releases in one order: lane threads, streams drained, lanes closed, staging, networks, the rest.
#include <thread>
#include <sched.h>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "api_internal.h"
#include "geom_math.h"
#include "onnx_import.h"
#include "image_decode.h"

using namespace rt;

std::string& rt::create_error() {
  static thread_local std::string e;
  return e;
}
const char* rt_results_json_impl(rt_results* r, int page, int stage);
#define RT_PAGE(r, page) ((r) && (page) >= 0 && (size_t)(page) < (r)->pages.size() ? &(r)->pages[(size_t)(page)] : nullptr)
// the page of a per-line result of the rec options, where `line` is one of the lines `per_line` holds an element for (else null)
template <class V>
static const rt_results::Page* page_of_line(const rt_results* r, int page, int line, V rt_results::Page::*per_line) {
  const rt_results::Page* p = RT_PAGE(r, page);
  return p && line >= 0 && (size_t)line < (p->*per_line).size() ? p : nullptr;
}

// a line's geometry for rt_debug_word_boxes / rt_debug_span_quad: the crop of box8 as plan_crop (session.cpp) derives it; false:
// an empty crop or a singular homography
static bool crop_geom(const float* box8, int T, int W, int resized_w, wb::WordGeom& g) {
  const gm::CropDims cd = gm::crop_dims(box8);
  if (cd.w <= 0 || cd.h <= 0 || !gm::projection_inverse(box8, cd.cw, cd.ch, g.inv)) return false;
  g.T = T; g.W = W; g.resized_w = resized_w;
  g.w_c = cd.rot ? cd.h : cd.w; g.h_c = cd.rot ? cd.w : cd.h;
  g.rot270 = cd.rot; g.w = cd.w; g.h = cd.h; g.cw = cd.cw; g.ch = cd.ch;
  return true;
}
// The entries without a session report through the caller's buffer: f() under the exception guard, its message into err [err_cap]
template <typename F>
static int guarded_into(char* err, size_t err_cap, F f) {
  try {
    f();
    return RT_OK;
  } catch (const RtError& e) {
    if (err && err_cap) snprintf(err, err_cap, "%s", e.what());
    return e.code;
  } catch (const std::exception& e) {
    if (err && err_cap) snprintf(err, err_cap, "%s", e.what());
    return RT_ERR_BACKEND;
  }
}
// The host decode pool: fn(i) for every page i < n on the CPUs this PROCESS may use (affinity mask capped by the cgroup quota -- the
// GPU box shows 256 logical CPUs to a pod that owns 16), shared among the ranks of the node (LOCAL_WORLD_SIZE: one process per
// GPU), at most 16 threads.  Rethrows the first failing page's error in page order, like the reference's `?`.
template <typename F>
static void decode_pool(int n, F fn) {
  std::vector<std::exception_ptr> errs((size_t)n);
  std::atomic<int> next{0};
  auto work = [&] {
    for (int i; (i = next.fetch_add(1)) < n;) {
      try { fn(i); } catch (...) { errs[(size_t)i] = std::current_exception(); }
    }
  };
  const int nt = std::max(1, std::min<int>(n, std::min<int>(16, rt_host_cpu_budget())));
  std::vector<std::thread> th;
  for (int t = 1; t < nt; t++) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
  for (auto& e : errs) if (e) std::rethrow_exception(e);
}

extern "C" {

void rt_config_default(rt_config* c) {
  if (!c) return;
  memset(c, 0, sizeof(*c));
  c->struct_size = (uint32_t)sizeof(rt_config);
  c->device_id = 0;
  c->max_side_len = 2000; c->min_side_len = 30;
  c->det_limit_side_len = 736; c->det_limit_type = 0;
  for (int i = 0; i < 3; i++) { c->det_mean[i] = 0.5f; c->det_std[i] = 0.5f; }
  c->det_scale = 1.0f / 255.0f;
  c->det_thresh = 0.3f; c->det_box_thresh = 0.5f; c->det_unclip_ratio = 1.6f;
  c->det_min_mini_box_size = 3; c->det_dilation = 1;
  c->cls_image_shape[0] = 3; c->cls_image_shape[1] = 48; c->cls_image_shape[2] = 192;
  c->cls_batch_num = 6; c->cls_thresh = 0.9f;
  c->rec_image_shape[0] = 3; c->rec_image_shape[1] = 48; c->rec_image_shape[2] = 320;
  c->rec_batch_num = 6;
  c->max_boxes_per_page = 0; c->det_sub_batch = 0; c->lanes = 0; c->dtype = RT_DTYPE_F32;
  c->det_score_mode = 0;
  c->rec_return_word_box = 0;
  c->rec_return_candidates = 0;
  c->crop_source = 0;
}

int rt_create(const rt_config* cfg, rt_session** out) {
  RT_REQUIRE(cfg && out, (rt_session*)nullptr, "rt_create: null argument");
  *out = nullptr;
  RT_REQUIRE(cfg->struct_size == sizeof(rt_config), (rt_session*)nullptr,
             "rt_config.struct_size does not match this library's rt_config: fill the struct with rt_config_default() of the same header");
  RT_REQUIRE(cfg->rec_batch_num > 0 && cfg->cls_batch_num > 0, (rt_session*)nullptr, "batch_num must be positive");
  RT_REQUIRE(cfg->cls_image_shape[0] == 3 && cfg->rec_image_shape[0] == 3 && cfg->rec_image_shape[1] == 48 &&
                 cfg->cls_image_shape[1] == 48 && cfg->cls_image_shape[2] == 192,
             (rt_session*)nullptr, "unsupported cls/rec image_shape for the PP-OCRv4 mobile graphs");
  RT_REQUIRE(cfg->lanes >= 0 && cfg->lanes <= 4, (rt_session*)nullptr, "lanes must be in [0, 4]");
  RT_REQUIRE(cfg->dtype == RT_DTYPE_F32 || cfg->dtype == RT_DTYPE_F16, (rt_session*)nullptr, "dtype must be RT_DTYPE_F32 or RT_DTYPE_F16");
  RT_REQUIRE(cfg->max_boxes_per_page >= 0 && cfg->max_boxes_per_page <= 65536, (rt_session*)nullptr,
             "max_boxes_per_page must be in [0, 65536]");
  RT_REQUIRE(cfg->det_score_mode == 0 || cfg->det_score_mode == 1, (rt_session*)nullptr, "det_score_mode must be 0 (Fast) or 1 (Slow)");
  RT_REQUIRE(cfg->rec_return_word_box == 0 || cfg->rec_return_word_box == 1, (rt_session*)nullptr,
             "rec_return_word_box must be 0 (off) or 1 (on)");
  RT_REQUIRE(cfg->rec_return_candidates >= 0 && cfg->rec_return_candidates <= RT_MAX_CANDIDATES, (rt_session*)nullptr,
             "rec_return_candidates must be in [0, 8] (0 = off, K = 1 .. RT_MAX_CANDIDATES)");
  RT_REQUIRE(cfg->crop_source == 0 || cfg->crop_source == 1, (rt_session*)nullptr, "crop_source must be 0 (Resized) or 1 (Original)");
  capture_variant_defaults();
  return guarded(nullptr, [&] { *out = rt_session_create(cfg); });
}
void rt_destroy(rt_session* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  for (auto& w : s->workers) w->shutdown();   // lanes finish what was submitted (tickets never waited for are leaked, not raced)
  s->workers.clear();
  quiesce(s);   // every lane's stream drained
  for (int l = 0; l < s->n_lanes(); l++) s->lane(l)->close();
  s->helpers.clear();
  s->free_stage();
  s->det.reset(); s->cls.reset(); s->rec.reset();
  if (s->d_word_raw) (void)hipFree(s->d_word_raw);
  delete s;   // (and with it the rec stores' device tables)
}
const char* rt_last_error(const rt_session* s) { return s ? s->last_error.c_str() : create_error().c_str(); }
const char* rt_version(void) { return "retto_hip 0.1.0 (gfx950)"; }

int rt_det(rt_session* s, const float* nchw, int n, int c, int h, int w, float* out) {
  RT_REQUIRE(s && nchw && out, s, "rt_det: null argument");
  if (c != 3 || n <= 0 || h <= 0 || w <= 0 || h % 32 || w % 32) { s->last_error = "rt_det: expected [n,3,h,w] with h,w multiples of 32"; return RT_ERR_SHAPE; }
  return guarded(s, [&] { s->det_forward(nchw, n, h, w, out); });
}
int rt_cls(rt_session* s, const float* nchw, int n, int c, int h, int w, float* out) {
  RT_REQUIRE(s && nchw && out, s, "rt_cls: null argument");
  if (c != 3 || n <= 0 || h != 48 || w != 192) { s->last_error = "rt_cls: expected [n,3,48,192]"; return RT_ERR_SHAPE; }
  return guarded(s, [&] { s->cls_forward(nchw, n, h, w, out); });
}
int rt_rec(rt_session* s, const float* nchw, int n, int c, int h, int w, float* out, int* t_out) {
  RT_REQUIRE(s, s, "rt_rec: null session");
  if (c != 3 || n <= 0 || h != 48 || w < 8) { s->last_error = "rt_rec: expected [n,3,48,w>=8]"; return RT_ERR_SHAPE; }
  RT_REQUIRE(out == nullptr || nchw != nullptr, s, "rt_rec: null input");
  return guarded(s, [&] { s->rec_forward(nchw, n, h, w, out, t_out); });
}
int rt_rec_ragged(rt_session* s, const float* nchw, int n, const int* widths, float* out, int* t_out) {
  RT_REQUIRE(s && widths && n > 0, s, "rt_rec_ragged: bad argument");
  RT_REQUIRE(out == nullptr || nchw != nullptr, s, "rt_rec_ragged: null input");
  return guarded(s, [&] { s->rec_forward_ragged(nchw, n, widths, out, t_out); });
}
int rt_rec_classes(const rt_session* s) { return s ? s->rec->classes() : 0; }
const char* rt_model_info(const rt_session* s) { return s ? s->model_info.c_str() : ""; }

int rt_resize_both_dims(const rt_session* s, int h, int w, int* out_h, int* out_w) {
  if (!s || !out_h || !out_w) return RT_ERR_INVALID;
  int plan[4];
  int n = gm::resize_both_plan(h, w, s->cfg.max_side_len, s->cfg.min_side_len, plan);
  *out_h = n ? plan[2 * (n - 1)] : h; *out_w = n ? plan[2 * (n - 1) + 1] : w;
  return RT_OK;
}
int rt_resize_both(rt_session* s, const uint8_t* rgb, int h, int w, uint8_t* out, int out_h, int out_w) {
  RT_REQUIRE(s && rgb && out && h > 0 && w > 0, s, "rt_resize_both: bad argument");
  return guarded(s, [&] { s->resize_both(rgb, h, w, out, out_h, out_w); });
}
int rt_det_input_dims(const rt_session* s, int h, int w, int* out_h, int* out_w) {
  if (!s || !out_h || !out_w) return RT_ERR_INVALID;
  gm::resize_either_dims(h, w, s->cfg.det_limit_type, s->cfg.det_limit_side_len, out_h, out_w);
  return RT_OK;
}
int rt_det_preprocess(rt_session* s, const uint8_t* rgb, int h, int w, float* out_nchw) {
  RT_REQUIRE(s && rgb && out_nchw && h > 0 && w > 0, s, "rt_det_preprocess: bad argument");
  return guarded(s, [&] { s->det_preprocess(rgb, h, w, out_nchw); });
}
int rt_det_postprocess(rt_session* s, const float* pred, int h, int w, int ori_h, int ori_w, float* boxes, float* scores,
                       int max_out, int* n_out) {
  RT_REQUIRE(s && pred && boxes && scores && n_out && h > 0 && w > 0, s, "rt_det_postprocess: bad argument");
  return guarded(s, [&] { s->det_postprocess(pred, h, w, ori_h, ori_w, boxes, scores, max_out, n_out); });
}
int rt_crop_dims(const float* boxes, int n, int* ws, int* hs) {
  if (!boxes || !ws || !hs) return RT_ERR_INVALID;
  for (int i = 0; i < n; i++) {
    gm::CropDims d = gm::crop_dims(boxes + 8 * i);
    ws[i] = d.rot ? d.h : d.w; hs[i] = d.rot ? d.w : d.h;
  }
  return RT_OK;
}
int rt_crop_images(rt_session* s, const uint8_t* rgb, int h, int w, const float* boxes, int n, uint8_t* out, size_t out_cap) {
  RT_REQUIRE(s && rgb && boxes && out && h > 0 && w > 0 && n >= 0, s, "rt_crop_images: bad argument");
  return guarded(s, [&] { s->crop_images(rgb, h, w, boxes, n, out, out_cap); });
}
int rt_debug_warp_crops(rt_session* s, const uint8_t* rgb, int h, int w, const float* boxes, int n, int form, uint8_t* out,
                        size_t out_cap) {
  RT_REQUIRE(s && rgb && boxes && out && h > 0 && w > 0 && n >= 0 && (form == 0 || form == 1), s, "rt_debug_warp_crops: bad argument");
  return guarded(s, [&] { s->crop_images(rgb, h, w, boxes, n, out, out_cap, form); });
}
int rt_scale_and_clip(float* boxes, int n, double bitmap_w, double bitmap_h, double ori_w, double ori_h) {
  if (!boxes) return RT_ERR_INVALID;
  for (int i = 0; i < n; i++) gm::scale_and_clip(boxes + 8 * i, bitmap_w, bitmap_h, ori_w, ori_h);
  return RT_OK;
}
int rt_resize_norm_width(int img_h, int img_w, float max_wh_ratio) { return gm::resize_norm_width(img_h, img_w, max_wh_ratio); }
int rt_resize_norm_image(rt_session* s, const uint8_t* crop, int h, int w, int ori_h, int ori_w, int img_h, int img_w,
                         float max_wh_ratio, float* out_chw) {
  RT_REQUIRE(s && crop && out_chw && h > 0 && w > 0 && img_h > 0, s, "rt_resize_norm_image: bad argument");
  return guarded(s, [&] { s->resize_norm_image(crop, h, w, ori_h, ori_w, img_h, img_w, max_wh_ratio, out_chw); });
}
int rt_ctc_decode(rt_session* s, const float* probs, int n, int t, int c, int32_t* idx, float* prob, int32_t* tokens,
                  int32_t* n_tokens, float* scores) {
  RT_REQUIRE(s && probs && idx && prob && tokens && n_tokens && scores && n > 0 && t > 0 && c > 0, s, "rt_ctc_decode: bad argument");
  return guarded(s, [&] { s->ctc_decode(probs, n, t, c, idx, prob, tokens, n_tokens, scores); });
}

int rt_run_batch(rt_session* s, const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages, int mem,
                 const float* const* det_map_override, rt_results** out) {
  RT_REQUIRE(s && out && n_pages >= 0 && (n_pages == 0 || (rgb && hs && ws)), s, "rt_run_batch: bad argument");
  RT_REQUIRE(mem == RT_MEM_HOST || mem == RT_MEM_DEVICE || mem == RT_MEM_HOST_MAPS_DEVICE, s, "rt_run_batch: bad mem kind");
  *out = nullptr;
  return guarded(s, [&] { *out = s->run_batch(s->call_of(rgb, hs, ws, n_pages, mem, det_map_override)); });
}
int rt_run_batch_stream(rt_session* s, const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages, int mem,
                        const float* const* det_map_override, rt_stage_callback cb, void* user, rt_results** out) {
  RT_REQUIRE(s && out && cb && n_pages >= 0 && (n_pages == 0 || (rgb && hs && ws)), s, "rt_run_batch_stream: bad argument");
  RT_REQUIRE(mem == RT_MEM_HOST || mem == RT_MEM_DEVICE || mem == RT_MEM_HOST_MAPS_DEVICE, s, "rt_run_batch_stream: bad mem kind");
  *out = nullptr;
  return guarded(s, [&] { *out = s->run_batch(s->call_of(rgb, hs, ws, n_pages, mem, det_map_override, cb, user)); });
}
// the five rt_run_regions* forms: `name` is the entry's own, ids = {charsets, lexicons, patterns, keywords}: an array it does not take is null
static int run_regions(const char* name, rt_session* s, const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages, int mem,
                       const float* const* quads, const int* n_quads, const int32_t* const* const (&ids)[REC_N_KINDS], rt_results** out) {
  RT_REQUIRE(s && out && n_pages >= 0 && (n_pages == 0 || (rgb && hs && ws && quads && n_quads)), s, std::string(name) + ": bad argument");
  RT_REQUIRE(mem == RT_MEM_HOST || mem == RT_MEM_DEVICE, s, std::string(name) + ": mem must be RT_MEM_HOST or RT_MEM_DEVICE");
  *out = nullptr;
  return guarded(s, [&] { *out = s->run_regions(rgb, hs, ws, n_pages, mem, quads, n_quads, ids); });
}
int rt_run_regions(rt_session* s, const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages, int mem,
                   const float* const* quads, const int* n_quads, rt_results** out) {
  return run_regions("rt_run_regions", s, rgb, hs, ws, n_pages, mem, quads, n_quads, {nullptr, nullptr, nullptr, nullptr}, out);
}
int rt_run_regions_charsets(rt_session* s, const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages, int mem,
                            const float* const* quads, const int* n_quads, const int32_t* const* charsets, rt_results** out) {
  return run_regions("rt_run_regions_charsets", s, rgb, hs, ws, n_pages, mem, quads, n_quads, {charsets, nullptr, nullptr, nullptr}, out);
}
int rt_run_regions_lexicons(rt_session* s, const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages, int mem,
                            const float* const* quads, const int* n_quads, const int32_t* const* charsets,
                            const int32_t* const* lexicons, rt_results** out) {
  return run_regions("rt_run_regions_lexicons", s, rgb, hs, ws, n_pages, mem, quads, n_quads, {charsets, lexicons, nullptr, nullptr}, out);
}
int rt_run_regions_patterns(rt_session* s, const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages, int mem,
                            const float* const* quads, const int* n_quads, const int32_t* const* charsets,
                            const int32_t* const* lexicons, const int32_t* const* patterns, rt_results** out) {
  return run_regions("rt_run_regions_patterns", s, rgb, hs, ws, n_pages, mem, quads, n_quads, {charsets, lexicons, patterns, nullptr}, out);
}
int rt_run_regions_keywords(rt_session* s, const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages, int mem,
                            const float* const* quads, const int* n_quads, const int32_t* const* charsets,
                            const int32_t* const* lexicons, const int32_t* const* patterns, const int32_t* const* keywords,
                            rt_results** out) {
  return run_regions("rt_run_regions_keywords", s, rgb, hs, ws, n_pages, mem, quads, n_quads, {charsets, lexicons, patterns, keywords}, out);
}
// rt_set_rec_charset / _lexicon / _pattern / _keywords: the session default of one kind (rec_line_opts.h)
static int set_rec_default(rt_session* s, const RecKind& kind, int id) {
  const std::string name = std::string("rt_set_rec_") + kind.noun;
  RT_REQUIRE(s, s, name + ": null session");
  return guarded(s, [&] {
    if (id < 0 || id > s->rec_counts().*kind.id) throw RtError(RT_ERR_INVALID, name + ": unknown " + kind.noun + " id " + std::to_string(id));
    s->rec_default.*kind.id = id;
  });
}
int rt_set_rec_charset(rt_session* s, int charset) { return set_rec_default(s, REC_KINDS[0], charset); }
int rt_set_rec_lexicon(rt_session* s, int lexicon) { return set_rec_default(s, REC_KINDS[1], lexicon); }
int rt_set_rec_pattern(rt_session* s, int pattern) { return set_rec_default(s, REC_KINDS[2], pattern); }
int rt_set_rec_keywords(rt_session* s, int list) { return set_rec_default(s, REC_KINDS[3], list); }
int rt_charset_create(rt_session* s, const char* utf8, size_t len, const int32_t* ids, int n_ids, int* charset_out) {
  RT_REQUIRE(s && charset_out && (utf8 || !len) && n_ids >= 0 && (ids || !n_ids), s, "rt_charset_create: bad argument");
  *charset_out = 0;
  return guarded(s, [&] { *charset_out = s->charset_create(utf8, len, ids, n_ids); });
}
int rt_charset_classes(const rt_session* s, int charset, const int32_t** ids) {
  if (!s || !s->charsets || charset < 1 || charset > (int)s->charsets->ids.size()) return 0;
  const std::vector<int32_t>& v = s->charsets->ids[(size_t)charset - 1];
  if (ids) *ids = v.data();
  return (int)v.size();
}
int rt_lexicon_create(rt_session* s, const char* utf8, size_t len, const int32_t* ids, const int32_t* entry_lens, int n_id_entries,
                      int* lexicon_out) {
  RT_REQUIRE(s && lexicon_out && (utf8 || !len) && n_id_entries >= 0 && ((ids && entry_lens) || !n_id_entries), s,
             "rt_lexicon_create: bad argument");
  *lexicon_out = 0;
  return guarded(s, [&] { *lexicon_out = s->lexicon_create(utf8, len, ids, entry_lens, n_id_entries); });
}
static const rt_entry_store::Host* lexicon_of(const rt_session* s, int lexicon) { return s && s->lexicons ? s->lexicons->list(lexicon) : nullptr; }
int rt_lexicon_entries(const rt_session* s, int lexicon) { return s && s->lexicons ? s->lexicons->entries(lexicon) : 0; }
int rt_lexicon_entry(const rt_session* s, int lexicon, int entry, const int32_t** ids) {
  return s && s->lexicons ? s->lexicons->entry(lexicon, entry, ids) : 0;
}
const char* rt_lexicon_entry_text(const rt_session* s, int lexicon, int entry) {
  return s && s->lexicons ? s->lexicons->entry_text(lexicon, entry) : nullptr;
}
int rt_keywords_create(rt_session* s, const char* utf8, size_t len, const int32_t* ids, const int32_t* entry_lens, int n_id_entries,
                       float min_score, int* list_out) {
  RT_REQUIRE(s && list_out && (utf8 || !len) && n_id_entries >= 0 && ((ids && entry_lens) || !n_id_entries), s,
             "rt_keywords_create: bad argument");
  *list_out = 0;
  return guarded(s, [&] { *list_out = s->keywords_create(utf8, len, ids, entry_lens, n_id_entries, min_score); });
}
static const rt_entry_store::Host* keywords_of(const rt_session* s, int list) { return s && s->keywords ? s->keywords->list(list) : nullptr; }
int rt_keywords_entries(const rt_session* s, int list) { return s && s->keywords ? s->keywords->entries(list) : 0; }
int rt_keywords_entry(const rt_session* s, int list, int entry, const int32_t** ids) {
  return s && s->keywords ? s->keywords->entry(list, entry, ids) : 0;
}
const char* rt_keywords_entry_text(const rt_session* s, int list, int entry) {
  return s && s->keywords ? s->keywords->entry_text(list, entry) : nullptr;
}
float rt_keywords_min_score(const rt_session* s, int list) {
  return keywords_of(s, list) ? s->keywords->min_score[(size_t)list - 1] : NAN;
}
int rt_pattern_create(rt_session* s, const char* utf8, size_t len, int* pattern_out) {
  RT_REQUIRE(s && pattern_out && (utf8 || len == 0), s, "rt_pattern_create: null argument");
  return guarded(s, [&] { *pattern_out = s->pattern_create(utf8 ? utf8 : "", len); });
}
static const rt_patterns::Host* pattern_of(const rt_session* s, int pattern) {
  if (!s || !s->patterns || pattern < 1 || pattern > (int)s->patterns->host.size()) return nullptr;
  return s->patterns->host[(size_t)pattern - 1].get();
}
int rt_pattern_info(const rt_session* s, int pattern, int* states, int* pairs, int* min_steps) {
  const rt_patterns::Host* h = pattern_of(s, pattern);
  if (!h) return RT_ERR_INVALID;
  if (states) *states = h->S;
  if (pairs) *pairs = h->P;
  if (min_steps) *min_steps = h->min_steps;
  return RT_OK;
}
const char* rt_pattern_text(const rt_session* s, int pattern) {
  const rt_patterns::Host* h = pattern_of(s, pattern);
  return h ? h->text.c_str() : nullptr;
}
int rt_results_rec_pattern(const rt_results* r, int page, int line, rt_pattern_result* out) {
  auto* p = page_of_line(r, page, line, &rt_results::Page::pat_id);
  if (!p || p->pat_id[(size_t)line] <= 0) return 0;
  const pt::LineResult& v = p->pat_res[(size_t)line];
  if (out) *out = rt_pattern_result{p->pat_id[(size_t)line], v.matched, v.logprob, v.free_logprob};
  return 1;
}
static_assert(RT_DET_MAX_PIXELS == dt::MAX_DET_PIXELS, "the header's det input limit is det_tiles.h's");
int rt_set_det_tiles(rt_session* s, int tile, int overlap) {
  RT_REQUIRE(s, s, "rt_set_det_tiles: null session");
  return guarded(s, [&] {
    if (const char* why = dt::check_params(tile, overlap)) throw RtError(RT_ERR_INVALID, std::string("rt_set_det_tiles: ") + why);
    s->det_tile = tile; s->det_overlap = overlap;
  });
}
int rt_det_tiles(const rt_session* s, int* tile, int* overlap) {
  if (!s) return RT_ERR_INVALID;
  if (tile) *tile = s->det_tile;
  if (overlap) *overlap = s->det_overlap;
  return RT_OK;
}
int rt_set_rec_beam(rt_session* s, int beam, int nbest) {
  RT_REQUIRE(s, s, "rt_set_rec_beam: null session");
  return guarded(s, [&] {
    if (beam == 0) { s->beam_b = s->beam_n = 0; return; }
    if (const char* why = bm::check_params(beam, nbest))
      throw RtError(RT_ERR_INVALID, "rt_set_rec_beam(" + std::to_string(beam) + ", " + std::to_string(nbest) + "): " + why);
    s->beam_b = beam; s->beam_n = nbest;
  });
}
int rt_rec_beam(const rt_session* s, int* beam, int* nbest) {
  if (!s) return RT_ERR_INVALID;
  if (beam) *beam = s->beam_b;
  if (nbest) *nbest = s->beam_n;
  return RT_OK;
}
int rt_lm_create(rt_session* s, const char* arpa, size_t len, float oov_log10, int* lm_out) {
  RT_REQUIRE(s && lm_out && (arpa || !len), s, "rt_lm_create: bad argument");
  *lm_out = -1;
  return guarded(s, [&] { *lm_out = s->lm_create(arpa, len, oov_log10); });
}
int rt_lm_info(const rt_session* s, int lm, int* order, int* ngrams, int* dropped, int* states) {
  if (!s || !s->lms || lm < 0 || lm >= (int)s->lms->host.size()) return RT_ERR_INVALID;
  const lm::Model& m = *s->lms->host[(size_t)lm];
  if (order) *order = m.order;
  if (ngrams) *ngrams = m.n_ngrams;
  if (dropped) *dropped = m.dropped;
  if (states) *states = (int)m.states.size();
  return RT_OK;
}
int rt_set_rec_beam_lm(rt_session* s, int lm, float alpha, float beta) {
  RT_REQUIRE(s, s, "rt_set_rec_beam_lm: null session");
  return guarded(s, [&] {
    if (lm == -1) { s->beam_lm = -1; s->lm_alpha = s->lm_beta = 0.0f; return; }
    if (lm < 0 || lm >= (int)s->lms->host.size())
      throw RtError(RT_ERR_INVALID, "rt_set_rec_beam_lm: " + std::to_string(lm) + " is not a language model of this session");
    if (const char* why = lm::check_weights(alpha, beta)) throw RtError(RT_ERR_INVALID, std::string("rt_set_rec_beam_lm: ") + why);
    s->beam_lm = lm; s->lm_alpha = alpha; s->lm_beta = beta;
  });
}
int rt_rec_beam_lm(const rt_session* s, int* lm, float* alpha, float* beta) {
  if (!s) return RT_ERR_INVALID;
  if (lm) *lm = s->beam_lm;
  if (alpha) *alpha = s->lm_alpha;
  if (beta) *beta = s->lm_beta;
  return RT_OK;
}
int rt_vocab_create(rt_session* s, const char* utf8, size_t len, const int32_t* ids, const int32_t* word_lens, int n_id_words, int flags,
                    int* vocab_out) {
  RT_REQUIRE(s && vocab_out && (utf8 || !len) && n_id_words >= 0 && ((ids && word_lens) || !n_id_words), s, "rt_vocab_create: bad argument");
  *vocab_out = -1;
  return guarded(s, [&] { *vocab_out = s->vocab_create(utf8, len, ids, word_lens, n_id_words, flags); });
}
int rt_vocab_info(const rt_session* s, int vocab, int* words, int* nodes, int* word_classes, int* variants_dropped) {
  if (!s || !s->vocabs || vocab < 0 || vocab >= (int)s->vocabs->host.size()) return RT_ERR_INVALID;
  const vc::Vocab& m = *s->vocabs->host[(size_t)vocab];
  if (words) *words = m.n_words;
  if (nodes) *nodes = (int)m.nodes.size();
  if (word_classes) *word_classes = m.n_word_classes;
  if (variants_dropped) *variants_dropped = m.variants_dropped;
  return RT_OK;
}
int rt_set_rec_beam_vocab(rt_session* s, int vocab, float gamma) {
  RT_REQUIRE(s, s, "rt_set_rec_beam_vocab: null session");
  return guarded(s, [&] {
    if (vocab == -1) { s->beam_vocab = -1; s->vocab_gamma = 0.0f; return; }
    if (vocab < 0 || vocab >= (int)s->vocabs->host.size())
      throw RtError(RT_ERR_INVALID, "rt_set_rec_beam_vocab: " + std::to_string(vocab) + " is not a vocabulary of this session");
    if (const char* why = vc::check_gamma(gamma)) throw RtError(RT_ERR_INVALID, std::string("rt_set_rec_beam_vocab: ") + why);
    s->beam_vocab = vocab; s->vocab_gamma = gamma;
  });
}
int rt_rec_beam_vocab(const rt_session* s, int* vocab, float* gamma) {
  if (!s) return RT_ERR_INVALID;
  if (vocab) *vocab = s->beam_vocab;
  if (gamma) *gamma = s->vocab_gamma;
  return RT_OK;
}
int rt_set_rec_windows(rt_session* s, int window, int overlap) {
  RT_REQUIRE(s, s, "rt_set_rec_windows: null session");
  return guarded(s, [&] {
    if (const char* why = rw::check_params(window, overlap)) throw RtError(RT_ERR_INVALID, std::string("rt_set_rec_windows: ") + why);
    s->rec_window = window; s->rec_overlap = overlap;
  });
}
int rt_rec_windows(const rt_session* s, int* window, int* overlap) {
  if (!s) return RT_ERR_INVALID;
  if (window) *window = s->rec_window;
  if (overlap) *overlap = s->rec_overlap;
  return RT_OK;
}
int rt_set_rec_flip(rt_session* s, float cls_below) {
  RT_REQUIRE(s, s, "rt_set_rec_flip: null session");
  return guarded(s, [&] {
    if (const char* why = rf::check_param(cls_below)) throw RtError(RT_ERR_INVALID, std::string("rt_set_rec_flip: ") + why);
    s->rec_flip_below = cls_below;   // (the helper lanes get it with every call: CallSettings)
  });
}
int rt_rec_flip(const rt_session* s, float* cls_below) {
  if (!s) return RT_ERR_INVALID;
  if (cls_below) *cls_below = s->rec_flip_below;
  return RT_OK;
}
int rt_rec_flip_choose(int ntok0, float score0, int ntok1, float score1) { return rf::choose(ntok0, score0, ntok1, score1); }
int rt_results_rec_flip(const rt_results* r, int page, int line, float* score0, float* score1) {
  const rt_results::Page* p = r && page >= 0 && (size_t)page < r->pages.size() ? &r->pages[(size_t)page] : nullptr;
  if (!p || line < 0 || (size_t)line >= p->flip_outcome.size() || p->flip_outcome[(size_t)line] == 0) return 0;
  if (score0) *score0 = p->flip_scores[2 * (size_t)line];
  if (score1) *score1 = p->flip_scores[2 * (size_t)line + 1];
  return p->flip_outcome[(size_t)line];
}
int rt_rec_window_plan(int L, int window, int overlap, int32_t* origin, int32_t* width, int32_t* bound, int cap, int* n, int* T) {
  return guarded(nullptr, [&] {
    if (const char* why = rw::check_params(window, overlap)) throw RtError(RT_ERR_INVALID, std::string("rt_rec_window_plan: ") + why);
    if (L < rw::STEP) throw RtError(RT_ERR_INVALID, "rt_rec_window_plan: L must be at least 8, not " + std::to_string(L));
    // (a line that is not windowed comes out as one unit [0, L) that owns all its steps)
    const rw::Plan p = rw::plan(L, window, overlap);
    if (n) *n = p.n();
    if (T) *T = p.T;
    if ((origin || width || bound) && cap < p.n()) throw RtError(RT_ERR_INVALID, "rt_rec_window_plan: cap is smaller than the " + std::to_string(p.n()) + " units");
    for (int i = 0; i < p.n(); i++) {
      if (origin) origin[i] = p.origin[(size_t)i];
      if (width) width[i] = p.width[(size_t)i];
      if (bound) bound[i] = p.bound[(size_t)i];
    }
  });
}
int rt_results_rec_windows(const rt_results* r, int page, int line) {
  auto* p = page_of_line(r, page, line, &rt_results::Page::rec_units);
  return p ? p->rec_units[(size_t)line] : 0;
}
int rt_det_tile_plan(int h, int w, int tile, int overlap, int32_t* row_origin, int32_t* row_bound, int row_cap, int32_t* col_origin,
                     int32_t* col_bound, int col_cap, int* n_rows, int* n_cols, int* tile_h, int* tile_w) {
  return guarded(nullptr, [&] {
    if (const char* why = dt::check_params(tile, overlap)) throw RtError(RT_ERR_INVALID, std::string("rt_det_tile_plan: ") + why);
    std::string why;
    const int rc = dt::check_page(h, w, &why);
    if (rc != dt::OK) throw RtError(rc, "rt_det_tile_plan: " + why);
    // (an axis the tile covers is one tile of the axis' length, so a page that is not tiled comes out as one tile)
    const dt::Axis R = dt::axis_plan(h, tile, overlap), C = dt::axis_plan(w, tile, overlap);
    if (n_rows) *n_rows = R.n();
    if (n_cols) *n_cols = C.n();
    if (tile_h) *tile_h = R.len;
    if (tile_w) *tile_w = C.len;
    if ((row_origin || row_bound) && row_cap < R.n()) throw RtError(RT_ERR_INVALID, "rt_det_tile_plan: row_cap is smaller than the " + std::to_string(R.n()) + " tile rows");
    if ((col_origin || col_bound) && col_cap < C.n()) throw RtError(RT_ERR_INVALID, "rt_det_tile_plan: col_cap is smaller than the " + std::to_string(C.n()) + " tile columns");
    for (int i = 0; i < R.n(); i++) { if (row_origin) row_origin[i] = R.origin[(size_t)i]; if (row_bound) row_bound[i] = R.bound[(size_t)i]; }
    for (int i = 0; i < C.n(); i++) { if (col_origin) col_origin[i] = C.origin[(size_t)i]; if (col_bound) col_bound[i] = C.bound[(size_t)i]; }
  });
}
int rt_lexicon_set_snap(rt_session* s, int lexicon, float min_posterior) {
  RT_REQUIRE(s, s, "rt_lexicon_set_snap: null session");
  return guarded(s, [&] { s->lexicon_set_snap(lexicon, min_posterior); });
}
float rt_lexicon_snap(const rt_session* s, int lexicon) {
  return lexicon_of(s, lexicon) ? s->lexicons->snap[lexicon - 1] : 0.0f;
}
int rt_submit_batch(rt_session* s, const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages, int mem,
                    const float* const* det_map_override, rt_ticket** out) {
  RT_REQUIRE(s && out && n_pages >= 0 && (n_pages == 0 || (rgb && hs && ws)), s, "rt_submit_batch: bad argument");
  RT_REQUIRE(mem == RT_MEM_HOST || mem == RT_MEM_DEVICE || mem == RT_MEM_HOST_MAPS_DEVICE, s, "rt_submit_batch: bad mem kind");
  RT_REQUIRE(s->inflight.load() < RT_MAX_INFLIGHT, s, "rt_submit_batch: too many batches in flight (RT_MAX_INFLIGHT)");
  *out = nullptr;
  return guarded<true>(s, [&] { *out = s->submit_batch(s->call_of(rgb, hs, ws, n_pages, mem, det_map_override)); });
}
int rt_wait_batch(rt_session* s, rt_ticket* ticket, rt_results** out) {
  RT_REQUIRE(s && ticket && out, s, "rt_wait_batch: bad argument");
  *out = nullptr;
  // (a failed batch: its own lanes have drained their streams in the worker; quiesce() in guarded() drains the rest)
  return guarded<true>(s, [&] { *out = s->wait_batch(ticket); });
}
int rt_host_cpu_budget(void) {
  int n = (int)std::thread::hardware_concurrency();
  cpu_set_t set;
  CPU_ZERO(&set);
  if (sched_getaffinity(0, sizeof(set), &set) == 0) { const int c = CPU_COUNT(&set); if (c > 0) n = c; }
  double quota = 0.0;
  if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {   // cgroup v2: "max <period>" or "<quota> <period>"
    char q[64]; double per = 0.0;
    if (fscanf(f, "%63s %lf", q, &per) == 2 && strcmp(q, "max") != 0 && per > 0) quota = atof(q) / per;
    fclose(f);
  } else {
    double q = -1, per = 0;
    if (FILE* fq = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (fscanf(fq, "%lf", &q) != 1) q = -1; fclose(fq); }
    if (FILE* fp = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(fp, "%lf", &per) != 1) per = 0; fclose(fp); }
    if (q > 0 && per > 0) quota = q / per;
  }
  if (quota > 0) n = std::max(1, std::min(n, (int)(quota + 0.5)));
  int ranks = 1;
  if (const char* e = getenv("LOCAL_WORLD_SIZE")) ranks = std::max(1, atoi(e));
  return std::max(1, n / ranks);
}
int rt_decode_image(const void* data, size_t len, uint8_t** rgb, int* h, int* w, char* err, size_t err_cap) {
  if (err && err_cap) err[0] = 0;
  if (!data || !rgb || !h || !w) { if (err && err_cap) snprintf(err, err_cap, "rt_decode_image: null argument"); return RT_ERR_INVALID; }
  *rgb = nullptr;
  return guarded_into(err, err_cap, [&] {
    std::vector<uint8_t> px;
    rt::decode_image((const uint8_t*)data, len, &px, h, w);
    uint8_t* p = (uint8_t*)malloc(px.size());
    if (!p) throw RtError(RT_ERR_BACKEND, "out of memory");
    memcpy(p, px.data(), px.size());
    *rgb = p;
  });
}
int rt_parse_dictionary(const void* data, size_t len, char** out, size_t* out_len, int* n_entries, char* err, size_t err_cap) {
  if (err && err_cap) err[0] = 0;
  if ((!data && len) || !out || !out_len || !n_entries) { if (err && err_cap) snprintf(err, err_cap, "rt_parse_dictionary: null argument"); return RT_ERR_INVALID; }
  *out = nullptr; *out_len = 0; *n_entries = 0;
  return guarded_into(err, err_cap, [&] {
    std::vector<uint8_t> bytes((const uint8_t*)data, (const uint8_t*)data + len);
    std::vector<std::string> d = rt::load_dictionary(bytes);
    std::string j;
    for (size_t i = 0; i < d.size(); i++) { if (i) j += '\n'; j += d[i]; }
    char* p = (char*)malloc(j.size() + 1);
    if (!p) throw RtError(RT_ERR_BACKEND, "out of memory");
    memcpy(p, j.data(), j.size()); p[j.size()] = 0;
    *out = p; *out_len = j.size(); *n_entries = (int)d.size();
  });
}
int rt_format_f32(float v, char* buf, size_t cap) {
  std::string s = rt_format_f32_impl(v);
  if (buf && cap) { size_t n = std::min(cap - 1, s.size()); memcpy(buf, s.data(), n); buf[n] = 0; }
  return (int)s.size();
}
// RettoSession::run / run_stream take the encoded bytes (session.rs:108,133): decode on host threads, then the batch path
int rt_run_encoded_batch(rt_session* s, const void* const* files, const size_t* lens, int n_pages, rt_stage_callback cb,
                         void* user, rt_results** out) {
  RT_REQUIRE(s && out && n_pages >= 0 && (n_pages == 0 || (files && lens)), s, "rt_run_encoded_batch: bad argument");
  *out = nullptr;
  return guarded(s, [&] {
    std::vector<std::vector<uint8_t>> px((size_t)n_pages);
    std::vector<int> hs((size_t)n_pages), ws((size_t)n_pages);
    decode_pool(n_pages, [&](int i) {
      if (!files[i]) throw RtError(RT_ERR_IMAGE, "image decode: null input");
      rt::decode_image((const uint8_t*)files[i], lens[i], &px[(size_t)i], &hs[(size_t)i], &ws[(size_t)i]);
    });
    std::vector<const uint8_t*> ptrs((size_t)n_pages);
    for (int i = 0; i < n_pages; i++) ptrs[(size_t)i] = px[(size_t)i].data();
    *out = s->run_batch(s->call_of(ptrs.data(), hs.data(), ws.data(), n_pages, RT_MEM_HOST, nullptr, cb, user));
  });
}
// The host stage of the device decode path: every page parsed and entropy-decoded (JPEG) or decoded (anything else) on the
// decode pool
static std::vector<rt::EncodedPage> host_stage(const void* const* files, const size_t* lens, int n_pages) {
  std::vector<rt::EncodedPage> enc((size_t)n_pages);
  decode_pool(n_pages, [&](int i) {
    if (!files[i]) throw RtError(RT_ERR_IMAGE, "image decode: null input");
    rt::decode_for_device((const uint8_t*)files[i], lens[i], &enc[(size_t)i]);
  });
  return enc;
}
int rt_submit_encoded_batch(rt_session* s, const void* const* files, const size_t* lens, int n_pages, rt_ticket** out) {
  if (out) *out = nullptr;
  RT_REQUIRE(s && out && n_pages >= 0 && (n_pages == 0 || (files && lens)), s, "rt_submit_encoded_batch: bad argument");
  RT_REQUIRE(s->inflight.load() < RT_MAX_INFLIGHT, s, "rt_submit_encoded_batch: too many batches in flight (RT_MAX_INFLIGHT)");
  return guarded<true>(s, [&] {
    std::vector<rt::EncodedPage> enc = host_stage(files, lens, n_pages);
    std::vector<const uint8_t*> rgb((size_t)n_pages, nullptr);
    std::vector<int> hs((size_t)n_pages), ws((size_t)n_pages);
    for (int i = 0; i < n_pages; i++) { hs[(size_t)i] = enc[(size_t)i].h; ws[(size_t)i] = enc[(size_t)i].w; }
    *out = s->submit_batch(s->call_of(rgb.data(), hs.data(), ws.data(), n_pages, RT_MEM_HOST), &enc);
  });
}
int rt_decode_batch(rt_session* s, const void* const* files, const size_t* lens, int n, int* hs, int* ws, uint8_t* const* out,
                    int mem, int* on_device) {
  RT_REQUIRE(s && n >= 0 && (n == 0 || (files && lens && hs && ws)), s, "rt_decode_batch: bad argument");
  RT_REQUIRE(!out || mem == RT_MEM_HOST || mem == RT_MEM_DEVICE, s, "rt_decode_batch: bad mem kind");
  for (int i = 0; out && i < n; i++) RT_REQUIRE(out[i], s, "rt_decode_batch: null output page");
  return guarded(s, [&] {
    if (!out) {
      for (int i = 0; i < n; i++) {
        if (!files[i]) throw RtError(RT_ERR_IMAGE, "image decode: null input");
        rt::image_dims((const uint8_t*)files[i], lens[i], &hs[i], &ws[i]);
        if (on_device) on_device[i] = 0;
      }
      return;
    }
    std::vector<rt::EncodedPage> enc = host_stage(files, lens, n);
    for (int i = 0; i < n; i++) {
      hs[i] = enc[(size_t)i].h; ws[i] = enc[(size_t)i].w;
      if (on_device) on_device[i] = enc[(size_t)i].on_device ? 1 : 0;
    }
    if (n) s->decode_batch(enc, out, mem);
  });
}
int rt_debug_jpeg_reconstruct(const void* data, size_t len, uint8_t** rgb, int* h, int* w, int* on_device, char* err,
                              size_t err_cap) {
  if (err && err_cap) err[0] = 0;
  if (!data || !rgb || !h || !w || !on_device) { if (err && err_cap) snprintf(err, err_cap, "rt_debug_jpeg_reconstruct: null argument"); return RT_ERR_INVALID; }
  *rgb = nullptr;
  return guarded_into(err, err_cap, [&] {
    rt::EncodedPage e;
    rt::decode_for_device((const uint8_t*)data, len, &e);
    if (e.on_device) rt::reconstruct_host(e.jpeg, &e.rgb);
    uint8_t* p = (uint8_t*)malloc(std::max<size_t>(e.rgb.size(), 1));
    if (!p) throw RtError(RT_ERR_BACKEND, "out of memory");
    memcpy(p, e.rgb.data(), e.rgb.size());
    *rgb = p; *h = e.h; *w = e.w; *on_device = e.on_device ? 1 : 0;
  });
}
void rt_results_free(rt_results* r) { delete r; }
int rt_results_pages(const rt_results* r) { return r ? (int)r->pages.size() : 0; }
int rt_results_count(const rt_results* r, int page) { auto* p = RT_PAGE(r, page); return p ? (int)p->det_scores.size() : 0; }
const float* rt_results_boxes(const rt_results* r, int page) { auto* p = RT_PAGE(r, page); return p ? p->boxes.data() : nullptr; }
const float* rt_results_det_scores(const rt_results* r, int page) { auto* p = RT_PAGE(r, page); return p ? p->det_scores.data() : nullptr; }
const uint16_t* rt_results_cls_labels(const rt_results* r, int page) { auto* p = RT_PAGE(r, page); return p ? p->cls_labels.data() : nullptr; }
const float* rt_results_cls_scores(const rt_results* r, int page) { auto* p = RT_PAGE(r, page); return p ? p->cls_scores.data() : nullptr; }
const float* rt_results_rec_scores(const rt_results* r, int page) { auto* p = RT_PAGE(r, page); return p ? p->rec_scores.data() : nullptr; }
int rt_results_rec_tokens(const rt_results* r, int page, int line, const int32_t** tokens) {
  auto* p = RT_PAGE(r, page);
  if (!p || line < 0 || (size_t)line >= p->tokens.size()) return 0;
  if (tokens) *tokens = p->tokens[(size_t)line].data();
  return (int)p->tokens[(size_t)line].size();
}
const char* rt_results_rec_text(const rt_results* r, int page, int line) {
  auto* p = RT_PAGE(r, page);
  if (!p || line < 0 || (size_t)line >= p->text.size()) return nullptr;
  return p->text[(size_t)line].c_str();
}
static_assert(sizeof(rt_word) == sizeof(wb::Word) && offsetof(rt_word, kind) == offsetof(wb::Word, kind),
              "rt_word and wb::Word must share one layout");
int rt_results_rec_words(const rt_results* r, int page, int line, const rt_word** words) {
  auto* p = RT_PAGE(r, page);
  if (!p || line < 0 || (size_t)line >= p->words.size()) return 0;
  if (words) *words = reinterpret_cast<const rt_word*>(p->words[(size_t)line].data());
  return (int)p->words[(size_t)line].size();
}
const char* rt_results_rec_word_text(rt_results* r, int page, int line, int word) {
  auto* p = RT_PAGE(r, page);
  if (!p || line < 0 || (size_t)line >= p->word_text.size()) return nullptr;
  const auto& wt = p->word_text[(size_t)line];
  if (word < 0 || (size_t)word >= wt.size()) return nullptr;
  return wt[(size_t)word].c_str();
}
int rt_debug_word_boxes(const void* dict, size_t dict_len, const int32_t* tokens, const int32_t* cols, int n, int T, int W,
                        int resized_w, const float* box8_after, int rot180, int after_w, int after_h, int ori_w, int ori_h,
                        rt_word* out, int* n_words) {
  if ((!dict && dict_len) || !box8_after || !n_words || n < 0 || (n > 0 && (!tokens || !cols || !out))) return RT_ERR_INVALID;
  if (T <= 0 || W <= 0 || after_w <= 0 || after_h <= 0 || ori_w <= 0 || ori_h <= 0) return RT_ERR_INVALID;
  *n_words = 0;
  try {
    std::vector<uint8_t> bytes((const uint8_t*)dict, (const uint8_t*)dict + dict_len);
    const std::vector<std::string> d = rt::load_dictionary(bytes);
    std::vector<uint8_t> raw(d.size());
    for (size_t i = 0; i < d.size(); i++) raw[i] = wb::raw_class(d[i].data(), d[i].size());
    for (int k = 0; k < n; k++) {
      if (tokens[k] < 0 || (size_t)tokens[k] >= d.size()) return RT_ERR_INVALID;
      if (cols[k] < 0 || cols[k] >= T || (k > 0 && cols[k] <= cols[k - 1])) return RT_ERR_INVALID;
    }
    wb::WordGeom g;
    if (!crop_geom(box8_after, T, W, resized_w, g)) return RT_ERR_IMAGE;
    wb::Word* o = reinterpret_cast<wb::Word*>(out);
    const int nw = wb::line_words(raw.data(), tokens, cols, n, g, rot180 ? 1 : 0, o);
    for (int j = 0; j < nw; j++) gm::scale_and_clip(o[j].quad, (double)after_w, (double)after_h, (double)ori_w, (double)ori_h);
    *n_words = nw;
    return RT_OK;
  } catch (const RtError& e) {
    return e.code;
  } catch (const std::exception&) {
    return RT_ERR_BACKEND;
  }
}
int rt_results_rec_candidates(const rt_results* r, int page, int line, const rt_candidate** cands, const int32_t** cols) {
  auto* p = RT_PAGE(r, page);
  if (!p || p->cand_k <= 0 || line < 0 || (size_t)line + 1 >= p->cand_off.size()) return 0;
  const size_t o = p->cand_off[(size_t)line];
  if (cands) *cands = reinterpret_cast<const rt_candidate*>(p->cands.data()) + o * (size_t)p->cand_k;
  if (cols) *cols = p->cand_cols.data() + o;
  return p->cand_k;
}
int rt_results_rec_lexicon(const rt_results* r, int page, int line, const rt_lexicon_match** m) {
  auto* p = page_of_line(r, page, line, &rt_results::Page::lex_n);
  if (!p) return 0;
  if (m) *m = reinterpret_cast<const rt_lexicon_match*>(p->lex_matches.data()) + (size_t)line * lx::MATCHES;
  return p->lex_n[(size_t)line];
}
int rt_results_rec_lexicon_id(const rt_results* r, int page, int line) {
  auto* p = page_of_line(r, page, line, &rt_results::Page::lex_id);
  return p ? p->lex_id[(size_t)line] : 0;
}
int rt_results_rec_lexicon_snapped(const rt_results* r, int page, int line) {
  auto* p = page_of_line(r, page, line, &rt_results::Page::lex_snapped);
  return p ? p->lex_snapped[(size_t)line] : 0;
}
int rt_results_rec_keywords(const rt_results* r, int page, int line, const rt_keyword_hit** hits) {
  auto* p = page_of_line(r, page, line, &rt_results::Page::kw_n);
  if (!p) return 0;
  if (hits) *hits = reinterpret_cast<const rt_keyword_hit*>(p->kw_hits.data()) + (size_t)line * kw::HITS;
  return p->kw_n[(size_t)line];
}
int rt_results_rec_keywords_id(const rt_results* r, int page, int line) {
  auto* p = page_of_line(r, page, line, &rt_results::Page::kw_id);
  return p ? p->kw_id[(size_t)line] : 0;
}
int rt_results_rec_beams(const rt_results* r, int page, int line, const rt_beam** out) {
  auto* p = page_of_line(r, page, line, &rt_results::Page::bm_count);
  if (!p || p->beam_n <= 0) return 0;
  if (out) *out = reinterpret_cast<const rt_beam*>(p->bm_recs.data()) + (size_t)line * p->beam_n;
  return p->bm_count[(size_t)line];
}
int rt_results_rec_beam_lm(const rt_results* r, int page, int line, const rt_beam_lm** out) {
  auto* p = page_of_line(r, page, line, &rt_results::Page::bm_count);
  if (!p || p->beam_n <= 0 || p->bm_lm.empty()) return 0;
  if (out) *out = reinterpret_cast<const rt_beam_lm*>(p->bm_lm.data()) + (size_t)line * p->beam_n;
  return p->bm_count[(size_t)line];
}
int rt_results_rec_beam_vocab(const rt_results* r, int page, int line, const rt_beam_vocab** out) {
  auto* p = page_of_line(r, page, line, &rt_results::Page::bm_count);
  if (!p || p->beam_n <= 0 || p->bm_vocab.empty()) return 0;
  if (out) *out = reinterpret_cast<const rt_beam_vocab*>(p->bm_vocab.data()) + (size_t)line * p->beam_n;
  return p->bm_count[(size_t)line];
}
int rt_results_rec_beam_tokens(const rt_results* r, int page, int line, int k, const int32_t** tokens) {
  auto* p = page_of_line(r, page, line, &rt_results::Page::bm_count);
  if (!p || p->beam_n <= 0 || k < 0 || k >= p->bm_count[(size_t)line]) return 0;
  const std::vector<int32_t>& t = p->bm_tokens[(size_t)line * p->beam_n + k];
  if (tokens) *tokens = t.data();
  return (int)t.size();
}
const char* rt_results_rec_beam_text(const rt_results* r, int page, int line, int k) {
  auto* p = page_of_line(r, page, line, &rt_results::Page::bm_count);
  if (!p || p->beam_n <= 0 || k < 0 || k >= p->bm_count[(size_t)line]) return nullptr;
  return p->bm_text[(size_t)line * p->beam_n + k].c_str();
}
int rt_debug_span_quad(int T, int W, int resized_w, const float* box8_after, int rot180, int after_w, int after_h, int ori_w, int ori_h,
                       int first_col, int last_col, float* quad8_out) {
  if (!box8_after || !quad8_out || T <= 0 || W <= 0 || resized_w <= 0 || after_w <= 0 || after_h <= 0 || ori_w <= 0 || ori_h <= 0)
    return RT_ERR_INVALID;
  if (first_col < 0 || last_col < first_col || last_col >= T) return RT_ERR_INVALID;
  wb::WordGeom g;
  if (!crop_geom(box8_after, T, W, resized_w, g)) return RT_ERR_IMAGE;
  kw::span_quad(first_col, last_col, g, rot180 ? 1 : 0, quad8_out);
  gm::scale_and_clip(quad8_out, (double)after_w, (double)after_h, (double)ori_w, (double)ori_h);
  return RT_OK;
}
double rt_results_det_checksum(const rt_results* r) { return r ? r->det_checksum : 0.0; }
const char* rt_results_json(rt_results* r, int page, int stage) {
  if (!RT_PAGE(r, page) || stage < 0 || stage > 2) return nullptr;
  return rt_results_json_impl(r, page, stage);
}

int rt_device_malloc(rt_session* s, size_t bytes, void** out) {
  RT_REQUIRE(s && out, s, "rt_device_malloc: null argument");
  return guarded(s, [&] { RT_HIP_CHECK(hipSetDevice(s->device)); RT_HIP_CHECK(hipMalloc(out, bytes)); });
}
int rt_device_free(rt_session* s, void* p) {
  RT_REQUIRE(s, s, "rt_device_free: null session");
  return guarded(s, [&] { RT_HIP_CHECK(hipSetDevice(s->device)); RT_HIP_CHECK(hipFree(p)); });
}
int rt_memcpy_h2d(rt_session* s, void* dst, const void* src, size_t bytes) {
  RT_REQUIRE(s && dst && src, s, "rt_memcpy_h2d: null argument");
  return guarded(s, [&] { RT_HIP_CHECK(hipSetDevice(s->device)); RT_HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); });
}
int rt_memcpy_d2h(rt_session* s, void* dst, const void* src, size_t bytes) {
  RT_REQUIRE(s && dst && src, s, "rt_memcpy_d2h: null argument");
  return guarded(s, [&] { RT_HIP_CHECK(hipSetDevice(s->device)); RT_HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); });
}
int rt_synchronize(rt_session* s) {
  RT_REQUIRE(s, s, "rt_synchronize: null session");
  return guarded(s, [&] { RT_HIP_CHECK(hipSetDevice(s->device)); RT_HIP_CHECK(hipDeviceSynchronize()); });
}
int rt_set_lanes(rt_session* s, int lanes) {
  RT_REQUIRE(s && lanes >= 1, s, "rt_set_lanes: bad argument");
  s->active_lanes = lanes;
  return RT_OK;
}
int rt_profile_enable(rt_session* s, int on) {
  RT_REQUIRE(s, s, "rt_profile_enable: null session");
  return guarded(s, [&] {
    const int mode = on == 2 ? 2 : (on != 0 ? 1 : 0);   // 2: the enclosing network scopes only
    for (int l = 0; l < s->n_lanes(); l++) { s->lane(l)->prof.clear(); s->lane(l)->prof.on = mode; }
  });
}
int rt_profile_get(rt_session* s, const char* const** names, const float** ms, const int** calls, int* n) {
  RT_REQUIRE(s && names && ms && calls && n, s, "rt_profile_get: null argument");
  for (int l = 1; l < s->n_lanes(); l++) s->prof.merge(s->lane(l)->prof);
  *names = s->prof.names.data(); *ms = s->prof.ms.data(); *calls = s->prof.calls.data(); *n = (int)s->prof.names.size();
  return RT_OK;
}

int rt_onnx_to_rtwb(int which, const void* onnx, size_t len, void** out, size_t* out_len, char* err, size_t err_cap) {
  if (err && err_cap) err[0] = 0;
  if (!onnx || !len || !out || !out_len) { if (err && err_cap) snprintf(err, err_cap, "rt_onnx_to_rtwb: null argument"); return RT_ERR_INVALID; }
  return guarded_into(err, err_cap, [&] {
    std::vector<uint8_t> b = rt::onnx_to_rtwb(which, (const uint8_t*)onnx, len);
    void* p = malloc(b.size());
    if (!p) throw RtError(RT_ERR_BACKEND, "out of memory");
    memcpy(p, b.data(), b.size());
    *out = p; *out_len = b.size();
  });
}
void rt_buffer_free(void* p) { free(p); }
size_t rt_model_manifest(int which, char* buf, size_t cap) {
  std::string s;
  try {
    for (const rt::ManifestEntry& m : rt::model_manifest(which)) {
      s += m.name;
      for (int d : m.dims) s += " " + std::to_string(d);
      s += "\n";
    }
  } catch (const std::exception&) { return 0; }
  if (buf && cap) { size_t n = std::min(cap - 1, s.size()); memcpy(buf, s.data(), n); buf[n] = 0; }
  return s.size() + 1;
}

}  // extern "C"
