// extern "C" surface of libretto_hip.so (include/retto_hip.h): sessions, the networks, the pipeline stages, batches, results,
// parsers and device memory, with the feature-level debug hooks that are thin forwards into their features (rt_debug_warp_crops,
// rt_debug_jpeg_reconstruct, rt_debug_word_boxes, rt_debug_ctc_candidates_host, rt_debug_charset_compile, rt_debug_ctc_charset_host, rt_debug_lexicon_compile, rt_debug_ctc_lexicon_host, rt_debug_ctc_lexicon_align_host, rt_debug_ctc_keywords_host, rt_debug_span_quad, rt_debug_ctc_beam_host).  The kernel-level diagnostics (rt_debug_set_variants,
// rt_bench_*, and the rt_debug_* harnesses the kernel tests drive) are in api_debug.cpp; api_internal.h holds what both share.
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
bool rt::cand_args_ok(const float* z5, const float* W, int N, const int32_t* idx, const float* prob, const int32_t* tokens_per_line,
                      int n_lines, int K, const rt_candidate* cands_out, const int32_t* cols_out, const int32_t* n_tokens_out,
                      long long* rows_out) {
  if (!idx || !prob || !tokens_per_line || !cands_out || !cols_out || !n_tokens_out) return false;
  if (n_lines <= 0 || K < 1 || K > RT_MAX_CANDIDATES || N <= 0 || (K > 1 && (!z5 || !W))) return false;
  long long rows = 0;
  for (int i = 0; i < n_lines; i++) {
    if (tokens_per_line[i] < 0) return false;
    rows += tokens_per_line[i];
  }
  if (rows >= (1ll << 30)) return false;
  for (long long r = 0; r < rows; r++)
    if (idx[r] < 0 || idx[r] >= N) return false;
  *rows_out = rows;
  return true;
}
bool rt::charset_args_ok(const float* z5, const float* W, int N, const int32_t* idx, const float* prob, const int32_t* tokens_per_line,
                         int n_lines, const int32_t* line_set, const uint32_t* masks, int n_sets, int K, const int32_t* tokens_out,
                         const int32_t* n_tokens_out, const float* scores_out, const rt_candidate* cands_out, const int32_t* cols_out,
                         long long* rows_out) {
  if (!z5 || !W || !idx || !prob || !tokens_per_line || !line_set || !tokens_out || !n_tokens_out || !scores_out) return false;
  if (n_lines <= 0 || N <= 0 || K < 0 || K > RT_MAX_CANDIDATES || n_sets < 0 || n_sets > RT_MAX_CHARSETS || (n_sets > 0 && !masks)) return false;
  if (K > 0 && (!cands_out || !cols_out)) return false;
  long long rows = 0;
  for (int i = 0; i < n_lines; i++) {
    if (tokens_per_line[i] < 0 || line_set[i] < 0 || line_set[i] > n_sets) return false;
    rows += tokens_per_line[i];
  }
  if (rows >= (1ll << 30)) return false;
  for (long long r = 0; r < rows; r++)
    if (idx[r] < 0 || idx[r] >= N) return false;
  *rows_out = rows;
  return true;
}
std::string rt::lexicon_args_error(const float* z5, const float* W, int N, const int32_t* tokens_per_line, int n_lines,
                                   const int32_t* line_lex, const int32_t* entry_ids, const int32_t* entry_lens,
                                   const int32_t* lex_first_entry, int n_lex, const rt_lexicon_match* matches_out,
                                   const int32_t* n_matches_out, long long* rows_out, long long* table_out) {
  auto S = [](long long v) { return std::to_string(v); };
  if (!z5 || !W || !tokens_per_line || !line_lex || !entry_ids || !entry_lens || !lex_first_entry || !matches_out || !n_matches_out)
    return "a required pointer is null";
  if (n_lines <= 0) return "n_lines must be positive";
  if (N <= 1) return "N must be at least 2 (the blank and one class)";
  if (n_lex < 1 || n_lex > RT_MAX_LEXICONS) return "n_lex = " + S(n_lex) + " is outside [1, RT_MAX_LEXICONS]";
  if (lex_first_entry[0] != 0) return "lex_first_entry[0] must be 0";
  for (int k = 0; k < n_lex; k++) {
    const long long n = (long long)lex_first_entry[k + 1] - lex_first_entry[k];
    if (n < 1 || n > RT_LEXICON_MAX_ENTRIES) return "lexicon " + S(k + 1) + " has " + S(n) + " entries, outside [1, RT_LEXICON_MAX_ENTRIES]";
  }
  long long o = 0;
  for (int j = 0; j < lex_first_entry[n_lex]; j++) {
    if (entry_lens[j] < 1 || entry_lens[j] > RT_LEXICON_MAX_LEN)
      return "entry " + S(j) + " has " + S(entry_lens[j]) + " ids, outside [1, RT_LEXICON_MAX_LEN]";
    for (int i = 0; i < entry_lens[j]; i++)
      if (entry_ids[o + i] < 1 || entry_ids[o + i] >= N)
        return "class id " + S(entry_ids[o + i]) + " in entry " + S(j) + " is outside [1, " + S(N) + ")";
    o += entry_lens[j];
  }
  long long rows = 0, table = 0;
  for (int i = 0; i < n_lines; i++) {
    if (tokens_per_line[i] < 0) return "line " + S(i) + " has a negative number of time steps";
    if (line_lex[i] < 0 || line_lex[i] > n_lex) return "line " + S(i) + " names lexicon " + S(line_lex[i]) + ", outside [0, " + S(n_lex) + "]";
    rows += tokens_per_line[i];
    if (line_lex[i] > 0) table += lex_first_entry[line_lex[i]] - lex_first_entry[line_lex[i] - 1];
  }
  if (rows >= (1ll << 30)) return "the lines have " + S(rows) + " time steps, 2^30 or more";
  if (table >= (1ll << 30)) return "the loglik table has " + S(table) + " floats, 2^30 or more";
  *rows_out = rows; *table_out = table;
  return std::string();
}
std::string rt::keywords_args_error(const float* z5, const float* W, int N, const int32_t* tokens_per_line, int n_lines,
                                    const int32_t* line_kw, const int32_t* entry_ids, const int32_t* entry_lens,
                                    const int32_t* kw_first_entry, int n_kw, const float* kw_min_score, const rt_keyword_hit* hits_out,
                                    const int32_t* n_hits_out, long long* rows_out, long long* table_out) {
  auto S = [](long long v) { return std::to_string(v); };
  if (!z5 || !W || !tokens_per_line || !line_kw || !entry_ids || !entry_lens || !kw_first_entry || !kw_min_score || !hits_out || !n_hits_out)
    return "a required pointer is null";
  if (n_lines <= 0) return "n_lines must be positive";
  if (N <= 1) return "N must be at least 2 (the blank and one class)";
  if (n_kw < 1 || n_kw > RT_MAX_KEYWORD_LISTS) return "n_kw = " + S(n_kw) + " is outside [1, RT_MAX_KEYWORD_LISTS]";
  if (kw_first_entry[0] != 0) return "kw_first_entry[0] must be 0";
  for (int k = 0; k < n_kw; k++) {
    const long long n = (long long)kw_first_entry[k + 1] - kw_first_entry[k];
    if (n < 1 || n > RT_LEXICON_MAX_ENTRIES) return "list " + S(k + 1) + " has " + S(n) + " entries, outside [1, RT_LEXICON_MAX_ENTRIES]";
    if (!(kw_min_score[k] <= 0.0f)) return "kw_min_score[" + S(k) + "] = " + std::to_string(kw_min_score[k]) + " is not a number at most 0";
  }
  long long o = 0;
  for (int j = 0; j < kw_first_entry[n_kw]; j++) {
    if (entry_lens[j] < 1 || entry_lens[j] > RT_LEXICON_MAX_LEN)
      return "entry " + S(j) + " has " + S(entry_lens[j]) + " ids, outside [1, RT_LEXICON_MAX_LEN]";
    for (int i = 0; i < entry_lens[j]; i++)
      if (entry_ids[o + i] < 1 || entry_ids[o + i] >= N)
        return "class id " + S(entry_ids[o + i]) + " in entry " + S(j) + " is outside [1, " + S(N) + ")";
    o += entry_lens[j];
  }
  long long rows = 0, table = 0;
  for (int i = 0; i < n_lines; i++) {
    if (tokens_per_line[i] < 0) return "line " + S(i) + " has a negative number of time steps";
    if (line_kw[i] < 0 || line_kw[i] > n_kw) return "line " + S(i) + " names list " + S(line_kw[i]) + ", outside [0, " + S(n_kw) + "]";
    rows += tokens_per_line[i];
    if (line_kw[i] > 0) table += kw_first_entry[line_kw[i]] - kw_first_entry[line_kw[i] - 1];
  }
  if (rows >= (1ll << 30)) return "the lines have " + S(rows) + " time steps, 2^30 or more";
  if (table > lx::MAX_GROUP_TABLE) return "the score table has " + S(table) + " entries, more than a group's table holds";
  *rows_out = rows; *table_out = table;
  return std::string();
}
std::string rt::beam_args_error(const float* z5, const float* W, int N, const int32_t* tokens_per_line, int n_lines, int beam, int nbest,
                                const int32_t* counts_out, const rt_beam* beams_out, const int32_t* tokens_out, long long* rows_out) {
  auto S = [](long long v) { return std::to_string(v); };
  if (!z5 || !W || !tokens_per_line || !counts_out || !beams_out || !tokens_out) return "a required pointer is null";
  if (n_lines < 0) return "n_lines is negative";
  if (N <= 1) return "N must be at least 2 (the blank and one class)";
  if (beam < 0 || beam > RT_MAX_BEAM) return "beam = " + S(beam) + " is outside [0, RT_MAX_BEAM]";
  if (beam > 0 && (nbest < 1 || nbest > std::min(beam, RT_MAX_NBEST)))
    return "nbest = " + S(nbest) + " is outside [1, min(beam, RT_MAX_NBEST)]";
  long long rows = 0;
  for (int i = 0; i < n_lines; i++) {
    if (tokens_per_line[i] < 0) return "line " + S(i) + " has a negative number of time steps";
    rows += tokens_per_line[i];
  }
  if (rows >= (1ll << 30)) return "the lines have " + S(rows) + " time steps, 2^30 or more";
  if (beam > 0 && n_lines + rows * beam > bm::MAX_GROUP_NODES)
    return "the lines need " + S(n_lines + rows * beam) + " trie nodes, more than a group's trie holds";
  *rows_out = rows;
  return std::string();
}
std::string rt::lexicon_align_args_error(const float* lex_min_post, int n_lex, const int32_t* idx, const float* prob,
                                         const int32_t* snapped_out, const float* vit_out) {
  if (!lex_min_post || !idx || !prob || !snapped_out || !vit_out) return "a required pointer is null";
  for (int k = 0; k < n_lex; k++)
    if (!(lex_min_post[k] >= 0.0f && lex_min_post[k] <= 1.0f))
      return "lex_min_post[" + std::to_string(k) + "] = " + std::to_string(lex_min_post[k]) + " is outside [0, 1]";
  return std::string();
}
std::string rt::pattern_args_error(const float* z5, const float* W, int N, const int32_t* tokens_per_line, int n_lines,
                                   const int32_t* line_pat, const int32_t* pat_S, const int32_t* pat_G, const int32_t* group_of,
                                   const int32_t* delta, const int32_t* accept, int n_pat, const int32_t* idx, const float* prob,
                                   const int32_t* matched_out, const float* vit_out, const float* logprob_out, const float* free_out,
                                   long long* rows_out, std::vector<pt::Rule>* rules_out) {
  auto S = [](long long v) { return std::to_string(v); };
  if (!z5 || !W || !tokens_per_line || !line_pat || !pat_S || !pat_G || !group_of || !delta || !accept || !idx || !prob ||
      !matched_out || !vit_out || !logprob_out || !free_out)
    return "a required pointer is null";
  if (n_lines <= 0) return "n_lines must be positive";
  if (N <= 1 || N > 65535) return "N must be in [2, 65535]";
  if (n_pat < 1 || n_pat > RT_MAX_PATTERNS) return "n_pat = " + S(n_pat) + " is outside [1, RT_MAX_PATTERNS]";
  rules_out->assign((size_t)n_pat, pt::Rule());
  size_t od = 0, oa = 0;
  for (int k = 0; k < n_pat; k++) {
    if (pat_S[k] < 1 || pat_S[k] > RT_PATTERN_MAX_STATES) return "pattern " + S(k + 1) + ": S = " + S(pat_S[k]) + " is outside [1, RT_PATTERN_MAX_STATES]";
    if (pat_G[k] < 1 || pat_G[k] > N) return "pattern " + S(k + 1) + ": G = " + S(pat_G[k]) + " is outside [1, N]";
    const std::string bad = (*rules_out)[(size_t)k].build(N, pat_S[k], pat_G[k], group_of + (size_t)k * N, delta + od, accept + oa);
    if (!bad.empty()) return "pattern " + S(k + 1) + ": " + bad;
    od += (size_t)pat_S[k] * pat_G[k]; oa += (size_t)pat_S[k];
  }
  long long rows = 0;
  for (int i = 0; i < n_lines; i++) {
    if (tokens_per_line[i] < 0) return "line " + S(i) + " has a negative number of time steps";
    if (line_pat[i] < 0 || line_pat[i] > n_pat) return "line " + S(i) + " names pattern " + S(line_pat[i]) + ", outside [0, " + S(n_pat) + "]";
    rows += tokens_per_line[i];
  }
  if (rows >= (1ll << 30)) return "the lines have " + S(rows) + " time steps, 2^30 or more";
  *rows_out = rows;
  return std::string();
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
  if (s->st) { (void)hipStreamSynchronize(s->st); }
  for (auto& h : s->helpers) {
    if (h->st) (void)hipStreamSynchronize(h->st);
    if (h->d_flags) (void)hipFree(h->d_flags);
    if (h->ev_block) (void)hipEventDestroy(h->ev_block);
    if (h->st_part) { rt::forget_stream(h->st_part); (void)hipStreamDestroy(h->st_part); }
    if (h->st_full) (void)hipStreamDestroy(h->st_full);
  }
  s->helpers.clear();
  s->free_stage();
  s->det.reset(); s->cls.reset(); s->rec.reset();
  if (s->d_flags) (void)hipFree(s->d_flags);
  if (s->d_word_raw) (void)hipFree(s->d_word_raw);
  if (s->ev_block) (void)hipEventDestroy(s->ev_block);
  if (s->st_part) { rt::forget_stream(s->st_part); (void)hipStreamDestroy(s->st_part); }
  if (s->st_full) (void)hipStreamDestroy(s->st_full);
  delete s;
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
  return guarded(s, [&] { *out = s->run_batch(rgb, hs, ws, n_pages, mem, det_map_override); });
}
int rt_run_batch_stream(rt_session* s, const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages, int mem,
                        const float* const* det_map_override, rt_stage_callback cb, void* user, rt_results** out) {
  RT_REQUIRE(s && out && cb && n_pages >= 0 && (n_pages == 0 || (rgb && hs && ws)), s, "rt_run_batch_stream: bad argument");
  RT_REQUIRE(mem == RT_MEM_HOST || mem == RT_MEM_DEVICE || mem == RT_MEM_HOST_MAPS_DEVICE, s, "rt_run_batch_stream: bad mem kind");
  *out = nullptr;
  return guarded(s, [&] { *out = s->run_batch(rgb, hs, ws, n_pages, mem, det_map_override, cb, user); });
}
// the five rt_run_regions* forms: `name` is the entry's own, an array it does not take is null
static int run_regions(const char* name, rt_session* s, const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages, int mem,
                       const float* const* quads, const int* n_quads, const int32_t* const* charsets, const int32_t* const* lexicons,
                       const int32_t* const* patterns, rt_results** out, const int32_t* const* keywords = nullptr) {
  RT_REQUIRE(s && out && n_pages >= 0 && (n_pages == 0 || (rgb && hs && ws && quads && n_quads)), s, std::string(name) + ": bad argument");
  RT_REQUIRE(mem == RT_MEM_HOST || mem == RT_MEM_DEVICE, s, std::string(name) + ": mem must be RT_MEM_HOST or RT_MEM_DEVICE");
  *out = nullptr;
  return guarded(s, [&] { *out = s->run_regions(rgb, hs, ws, n_pages, mem, quads, n_quads, charsets, lexicons, patterns, keywords); });
}
int rt_run_regions(rt_session* s, const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages, int mem,
                   const float* const* quads, const int* n_quads, rt_results** out) {
  return run_regions("rt_run_regions", s, rgb, hs, ws, n_pages, mem, quads, n_quads, nullptr, nullptr, nullptr, out);
}
int rt_run_regions_charsets(rt_session* s, const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages, int mem,
                            const float* const* quads, const int* n_quads, const int32_t* const* charsets, rt_results** out) {
  return run_regions("rt_run_regions_charsets", s, rgb, hs, ws, n_pages, mem, quads, n_quads, charsets, nullptr, nullptr, out);
}
int rt_run_regions_lexicons(rt_session* s, const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages, int mem,
                            const float* const* quads, const int* n_quads, const int32_t* const* charsets,
                            const int32_t* const* lexicons, rt_results** out) {
  return run_regions("rt_run_regions_lexicons", s, rgb, hs, ws, n_pages, mem, quads, n_quads, charsets, lexicons, nullptr, out);
}
int rt_run_regions_patterns(rt_session* s, const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages, int mem,
                            const float* const* quads, const int* n_quads, const int32_t* const* charsets,
                            const int32_t* const* lexicons, const int32_t* const* patterns, rt_results** out) {
  return run_regions("rt_run_regions_patterns", s, rgb, hs, ws, n_pages, mem, quads, n_quads, charsets, lexicons, patterns, out);
}
int rt_run_regions_keywords(rt_session* s, const uint8_t* const* rgb, const int* hs, const int* ws, int n_pages, int mem,
                            const float* const* quads, const int* n_quads, const int32_t* const* charsets,
                            const int32_t* const* lexicons, const int32_t* const* patterns, const int32_t* const* keywords,
                            rt_results** out) {
  return run_regions("rt_run_regions_keywords", s, rgb, hs, ws, n_pages, mem, quads, n_quads, charsets, lexicons, patterns, out, keywords);
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
  const rt_results::Page* p = r && page >= 0 && (size_t)page < r->pages.size() ? &r->pages[(size_t)page] : nullptr;
  if (!p || line < 0 || (size_t)line >= p->pat_id.size() || p->pat_id[(size_t)line] <= 0) return 0;
  const pt::LineResult& v = p->pat_res[(size_t)line];
  if (out) *out = rt_pattern_result{p->pat_id[(size_t)line], v.matched, v.logprob, v.free_logprob};
  return 1;
}
static_assert(RT_DET_MAX_PIXELS == dt::MAX_DET_PIXELS, "the header's det input limit is det_tiles.h's");
int rt_set_det_tiles(rt_session* s, int tile, int overlap) {
  RT_REQUIRE(s, s, "rt_set_det_tiles: null session");
  return guarded(s, [&] {
    if (const char* why = dt::check_params(tile, overlap)) throw RtError(RT_ERR_INVALID, std::string("rt_set_det_tiles: ") + why);
    s->det_tile = tile; s->det_overlap = overlap;   // (the helper lanes get it with every call: CallSettings)
  });
}
int rt_det_tiles(const rt_session* s, int* tile, int* overlap) {
  if (!s) return RT_ERR_INVALID;
  if (tile) *tile = s->det_tile;
  if (overlap) *overlap = s->det_overlap;
  return RT_OK;
}
static_assert(RT_MAX_BEAM == bm::MAX_BEAM && RT_MAX_NBEST == bm::MAX_NBEST, "the RT_MAX_BEAM / RT_MAX_NBEST limits and bm:: must agree");
static_assert(sizeof(rt_beam) == sizeof(bm::Beam) && offsetof(rt_beam, logprob) == offsetof(bm::Beam, logprob) &&
                  offsetof(rt_beam, n_tokens) == offsetof(bm::Beam, n_tokens), "rt_beam and bm::Beam must share one layout");
int rt_set_rec_beam(rt_session* s, int beam, int nbest) {
  RT_REQUIRE(s, s, "rt_set_rec_beam: null session");
  return guarded(s, [&] {
    if (beam == 0) { s->beam_b = s->beam_n = 0; return; }
    if (const char* why = bm::check_params(beam, nbest))
      throw RtError(RT_ERR_INVALID, "rt_set_rec_beam(" + std::to_string(beam) + ", " + std::to_string(nbest) + "): " + why);
    s->beam_b = beam; s->beam_n = nbest;   // (the helper lanes get it with every call: CallSettings)
  });
}
int rt_rec_beam(const rt_session* s, int* beam, int* nbest) {
  if (!s) return RT_ERR_INVALID;
  if (beam) *beam = s->beam_b;
  if (nbest) *nbest = s->beam_n;
  return RT_OK;
}
int rt_set_rec_windows(rt_session* s, int window, int overlap) {
  RT_REQUIRE(s, s, "rt_set_rec_windows: null session");
  return guarded(s, [&] {
    if (const char* why = rw::check_params(window, overlap)) throw RtError(RT_ERR_INVALID, std::string("rt_set_rec_windows: ") + why);
    s->rec_window = window; s->rec_overlap = overlap;   // (the helper lanes get it with every call: CallSettings)
  });
}
int rt_rec_windows(const rt_session* s, int* window, int* overlap) {
  if (!s) return RT_ERR_INVALID;
  if (window) *window = s->rec_window;
  if (overlap) *overlap = s->rec_overlap;
  return RT_OK;
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
  const rt_results::Page* p = r && page >= 0 && (size_t)page < r->pages.size() ? &r->pages[(size_t)page] : nullptr;
  if (!p || line < 0 || (size_t)line >= p->rec_units.size()) return 0;
  return p->rec_units[(size_t)line];
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
  return guarded<true>(s, [&] { *out = s->submit_batch(rgb, hs, ws, n_pages, mem, det_map_override); });
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
  try {
    std::vector<uint8_t> px;
    rt::decode_image((const uint8_t*)data, len, &px, h, w);
    uint8_t* p = (uint8_t*)malloc(px.size());
    if (!p) throw RtError(RT_ERR_BACKEND, "out of memory");
    memcpy(p, px.data(), px.size());
    *rgb = p;
    return RT_OK;
  } catch (const RtError& e) {
    if (err && err_cap) snprintf(err, err_cap, "%s", e.what());
    return e.code;
  } catch (const std::exception& e) {
    if (err && err_cap) snprintf(err, err_cap, "%s", e.what());
    return RT_ERR_BACKEND;
  }
}
int rt_parse_dictionary(const void* data, size_t len, char** out, size_t* out_len, int* n_entries, char* err, size_t err_cap) {
  if (err && err_cap) err[0] = 0;
  if ((!data && len) || !out || !out_len || !n_entries) { if (err && err_cap) snprintf(err, err_cap, "rt_parse_dictionary: null argument"); return RT_ERR_INVALID; }
  *out = nullptr; *out_len = 0; *n_entries = 0;
  try {
    std::vector<uint8_t> bytes((const uint8_t*)data, (const uint8_t*)data + len);
    std::vector<std::string> d = rt::load_dictionary(bytes);
    std::string j;
    for (size_t i = 0; i < d.size(); i++) { if (i) j += '\n'; j += d[i]; }
    char* p = (char*)malloc(j.size() + 1);
    if (!p) throw RtError(RT_ERR_BACKEND, "out of memory");
    memcpy(p, j.data(), j.size()); p[j.size()] = 0;
    *out = p; *out_len = j.size(); *n_entries = (int)d.size();
    return RT_OK;
  } catch (const RtError& e) {
    if (err && err_cap) snprintf(err, err_cap, "%s", e.what());
    return e.code;
  } catch (const std::exception& e) {
    if (err && err_cap) snprintf(err, err_cap, "%s", e.what());
    return RT_ERR_BACKEND;
  }
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
    std::vector<std::exception_ptr> errs((size_t)n_pages);
    std::atomic<int> next{0};
    auto work = [&] {
      for (int i; (i = next.fetch_add(1)) < n_pages;) {
        try {
          if (!files[i]) throw RtError(RT_ERR_IMAGE, "image decode: null input");
          rt::decode_image((const uint8_t*)files[i], lens[i], &px[(size_t)i], &hs[(size_t)i], &ws[(size_t)i]);
        } catch (...) { errs[(size_t)i] = std::current_exception(); }
      }
    };
    // decode threads: the CPUs this PROCESS may use (affinity mask capped by the cgroup quota -- the GPU box shows 256 logical
    // CPUs to a pod that owns 16), shared among the ranks of the node (LOCAL_WORLD_SIZE: one process per GPU), at most 16
    const int nt = std::max(1, std::min<int>(n_pages, std::min<int>(16, rt_host_cpu_budget())));
    std::vector<std::thread> th;
    for (int t = 1; t < nt; t++) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
    for (auto& e : errs) if (e) std::rethrow_exception(e);  // first failing page in page order, like the reference's `?`
    std::vector<const uint8_t*> ptrs((size_t)n_pages);
    for (int i = 0; i < n_pages; i++) ptrs[(size_t)i] = px[(size_t)i].data();
    *out = s->run_batch(ptrs.data(), hs.data(), ws.data(), n_pages, RT_MEM_HOST, nullptr, cb, user);
  });
}
// The host stage of the device decode path: every page parsed and entropy-decoded (JPEG) or decoded (anything else) on the
// same thread pool as rt_run_encoded_batch; the first failing page in page order is reported.
static std::vector<rt::EncodedPage> host_stage(const void* const* files, const size_t* lens, int n_pages) {
  std::vector<rt::EncodedPage> enc((size_t)n_pages);
  std::vector<std::exception_ptr> errs((size_t)n_pages);
  std::atomic<int> next{0};
  auto work = [&] {
    for (int i; (i = next.fetch_add(1)) < n_pages;) {
      try {
        if (!files[i]) throw RtError(RT_ERR_IMAGE, "image decode: null input");
        rt::decode_for_device((const uint8_t*)files[i], lens[i], &enc[(size_t)i]);
      } catch (...) { errs[(size_t)i] = std::current_exception(); }
    }
  };
  const int nt = std::max(1, std::min<int>(n_pages, std::min<int>(16, rt_host_cpu_budget())));
  std::vector<std::thread> th;
  for (int t = 1; t < nt; t++) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
  for (auto& e : errs) if (e) std::rethrow_exception(e);
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
    *out = s->submit_batch(rgb.data(), hs.data(), ws.data(), n_pages, RT_MEM_HOST, nullptr, nullptr, nullptr, &enc);
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
  try {
    rt::EncodedPage e;
    rt::decode_for_device((const uint8_t*)data, len, &e);
    if (e.on_device) rt::reconstruct_host(e.jpeg, &e.rgb);
    uint8_t* p = (uint8_t*)malloc(std::max<size_t>(e.rgb.size(), 1));
    if (!p) throw RtError(RT_ERR_BACKEND, "out of memory");
    memcpy(p, e.rgb.data(), e.rgb.size());
    *rgb = p; *h = e.h; *w = e.w; *on_device = e.on_device ? 1 : 0;
    return RT_OK;
  } catch (const RtError& e) {
    if (err && err_cap) snprintf(err, err_cap, "%s", e.what());
    return e.code;
  } catch (const std::exception& e) {
    if (err && err_cap) snprintf(err, err_cap, "%s", e.what());
    return RT_ERR_BACKEND;
  }
}
void rt_results_free(rt_results* r) { delete r; }
int rt_results_pages(const rt_results* r) { return r ? (int)r->pages.size() : 0; }
#define RT_PAGE(r, page) ((r) && (page) >= 0 && (size_t)(page) < (r)->pages.size() ? &(r)->pages[(size_t)(page)] : nullptr)
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
    // the crop as plan_crops (session.cpp) derives it
    const gm::CropDims cd = gm::crop_dims(box8_after);
    if (cd.w <= 0 || cd.h <= 0) return RT_ERR_IMAGE;
    wb::WordGeom g;
    if (!gm::projection_inverse(box8_after, cd.cw, cd.ch, g.inv)) return RT_ERR_IMAGE;
    g.T = T; g.W = W; g.resized_w = resized_w;
    g.w_c = cd.rot ? cd.h : cd.w; g.h_c = cd.rot ? cd.w : cd.h;
    g.rot270 = cd.rot; g.w = cd.w; g.h = cd.h; g.cw = cd.cw; g.ch = cd.ch;
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
static_assert(sizeof(rt_candidate) == sizeof(cc::Cand) && offsetof(rt_candidate, prob) == offsetof(cc::Cand, prob) &&
                  RT_MAX_CANDIDATES == cc::MAX_K, "rt_candidate and cc::Cand must share one layout");
int rt_results_rec_candidates(const rt_results* r, int page, int line, const rt_candidate** cands, const int32_t** cols) {
  auto* p = RT_PAGE(r, page);
  if (!p || p->cand_k <= 0 || line < 0 || (size_t)line + 1 >= p->cand_off.size()) return 0;
  const size_t o = p->cand_off[(size_t)line];
  if (cands) *cands = reinterpret_cast<const rt_candidate*>(p->cands.data()) + o * (size_t)p->cand_k;
  if (cols) *cols = p->cand_cols.data() + o;
  return p->cand_k;
}
int rt_debug_ctc_candidates_host(const float* z5, const float* W, const float* bias, int N, const int32_t* idx, const float* prob,
                                 const int32_t* tokens_per_line, int n_lines, int K, rt_candidate* cands_out, int32_t* cols_out,
                                 int32_t* n_tokens_out) {
  long long rows = 0;
  if (!cand_args_ok(z5, W, N, idx, prob, tokens_per_line, n_lines, K, cands_out, cols_out, n_tokens_out, &rows)) return RT_ERR_INVALID;
  try {
    const int D = 120;
    std::vector<float> logits((size_t)N);
    cc::Cand* out = reinterpret_cast<cc::Cand*>(cands_out);
    long long o = 0;
    for (int i = 0; i < n_lines; i++) {
      const int T = tokens_per_line[i];
      const int n = cc::line_kept(idx + o, prob + o, T, K, cols_out + o, out + o * K);
      n_tokens_out[i] = n;
      for (int j = 0; K > 1 && j < n; j++) {
        cc::Cand* c = out + (o + j) * K;
        cc::row_candidates(z5 + (size_t)(o + cols_out[o + j]) * D, D, W, bias, N, c[0].id, K, c, logits.data());
      }
      o += T;
    }
    return RT_OK;
  } catch (const std::exception&) {
    return RT_ERR_BACKEND;
  }
}
static_assert(RT_MAX_CHARSETS == cs::MAX_SETS, "RT_MAX_CHARSETS and cs::MAX_SETS must agree");
int rt_debug_charset_compile(const void* dict, size_t dict_len, const char* utf8, size_t len, const int32_t* ids, int n_ids,
                             uint32_t* mask_out, int mask_cap, int* n_classes, char* err, size_t err_cap) {
  if (err && err_cap) err[0] = 0;
  if ((!dict && dict_len) || (!utf8 && len) || n_ids < 0 || (!ids && n_ids) || !n_classes || mask_cap < 0 || (!mask_out && mask_cap)) {
    if (err && err_cap) snprintf(err, err_cap, "rt_debug_charset_compile: bad argument");
    return RT_ERR_INVALID;
  }
  *n_classes = 0;
  try {
    std::vector<uint8_t> bytes((const uint8_t*)dict, (const uint8_t*)dict + dict_len);
    const std::vector<std::string> d = rt::load_dictionary(bytes);
    const std::vector<uint32_t> mask = rt::compile_charset(d, utf8, len, ids, n_ids);
    *n_classes = (int)d.size();
    if ((size_t)mask_cap < mask.size()) throw RtError(RT_ERR_INVALID, "rt_debug_charset_compile: the mask needs " + std::to_string(mask.size()) + " words");
    memcpy(mask_out, mask.data(), mask.size() * sizeof(uint32_t));
    return RT_OK;
  } catch (const RtError& e) {
    if (err && err_cap) snprintf(err, err_cap, "%s", e.what());
    return e.code;
  } catch (const std::exception& e) {
    if (err && err_cap) snprintf(err, err_cap, "%s", e.what());
    return RT_ERR_BACKEND;
  }
}
int rt_debug_ctc_charset_host(const float* z5, const float* W, const float* bias, int N, int32_t* idx, float* prob,
                              const int32_t* tokens_per_line, int n_lines, const int32_t* line_set, const uint32_t* masks,
                              int n_sets, int K, int32_t* tokens_out, int32_t* n_tokens_out, float* scores_out,
                              rt_candidate* cands_out, int32_t* cols_out) {
  long long rows = 0;
  if (!charset_args_ok(z5, W, N, idx, prob, tokens_per_line, n_lines, line_set, masks, n_sets, K, tokens_out, n_tokens_out,
                       scores_out, cands_out, cols_out, &rows))
    return RT_ERR_INVALID;
  try {
    const int D = 120, words = cs::mask_words(N);
    std::vector<float> logits((size_t)N);
    cc::Cand* out = reinterpret_cast<cc::Cand*>(cands_out);
    long long o = 0;
    for (int i = 0; i < n_lines; i++) {
      const int T = tokens_per_line[i];
      const uint32_t* m = line_set[i] > 0 ? masks + (size_t)(line_set[i] - 1) * words : nullptr;
      for (int t = 0; m && t < T; t++) {   // the restricted rows' (idx, prob), before the decode
        cs::row_logits(z5 + (size_t)(o + t) * D, D, W, bias, N, logits.data());
        cs::row_argmax(logits.data(), N, m, idx + o + t, prob + o + t, nullptr, nullptr);
      }
      int cnt = 0; float acc = 0.0f;   // k_ctc_decode
      for (int t = 0; t < T; t++)
        if (cc::kept(idx[o + t], t > 0 ? idx[o + t - 1] : 0, t == 0)) { tokens_out[o + cnt] = idx[o + t]; acc = acc + prob[o + t]; cnt++; }
      n_tokens_out[i] = cnt;
      scores_out[i] = acc / (float)(unsigned)cnt;
      if (K > 0) {
        const int n = cc::line_kept(idx + o, prob + o, T, K, cols_out + o, out + o * K);
        for (int j = 0; K > 1 && j < n; j++) {
          cc::Cand* c = out + (o + j) * K;
          const float* z = z5 + (size_t)(o + cols_out[o + j]) * D;
          if (m) { cs::row_logits(z, D, W, bias, N, logits.data()); cs::row_candidates(logits.data(), N, m, c[0].id, K, c); }
          else cc::row_candidates(z, D, W, bias, N, c[0].id, K, c, logits.data());
        }
      }
      o += T;
    }
    return RT_OK;
  } catch (const std::exception&) {
    return RT_ERR_BACKEND;
  }
}
static_assert(RT_MAX_LEXICONS == lx::MAX_LEXICONS && RT_LEXICON_MAX_ENTRIES == lx::MAX_ENTRIES && RT_LEXICON_MAX_LEN == lx::MAX_LEN &&
                  RT_LEXICON_MATCHES == lx::MATCHES, "the RT_LEXICON_* limits and lx:: must agree");
static_assert(sizeof(rt_lexicon_match) == sizeof(lx::Match) && offsetof(rt_lexicon_match, loglik) == offsetof(lx::Match, loglik) &&
                  offsetof(rt_lexicon_match, posterior) == offsetof(lx::Match, posterior), "rt_lexicon_match and lx::Match must share one layout");
int rt_results_rec_lexicon(const rt_results* r, int page, int line, const rt_lexicon_match** m) {
  auto* p = RT_PAGE(r, page);
  if (!p || line < 0 || (size_t)line >= p->lex_n.size()) return 0;
  if (m) *m = reinterpret_cast<const rt_lexicon_match*>(p->lex_matches.data()) + (size_t)line * lx::MATCHES;
  return p->lex_n[(size_t)line];
}
int rt_results_rec_lexicon_id(const rt_results* r, int page, int line) {
  auto* p = RT_PAGE(r, page);
  if (!p || line < 0 || (size_t)line >= p->lex_id.size()) return 0;
  return p->lex_id[(size_t)line];
}
int rt_results_rec_lexicon_snapped(const rt_results* r, int page, int line) {
  auto* p = RT_PAGE(r, page);
  if (!p || line < 0 || (size_t)line >= p->lex_snapped.size()) return 0;
  return p->lex_snapped[(size_t)line];
}
int rt_debug_lexicon_compile(const void* dict, size_t dict_len, const char* utf8, size_t len, const int32_t* ids,
                             const int32_t* entry_lens, int n_id_entries, int32_t* ids_out, int ids_cap, int32_t* lens_out,
                             int lens_cap, int* n_ids_out, int* n_entries_out, int* n_classes, char* err, size_t err_cap) {
  if (err && err_cap) err[0] = 0;
  if ((!dict && dict_len) || (!utf8 && len) || n_id_entries < 0 || ((!ids || !entry_lens) && n_id_entries) || !n_ids_out ||
      !n_entries_out || !n_classes || ids_cap < 0 || lens_cap < 0 || (!ids_out && ids_cap) || (!lens_out && lens_cap)) {
    if (err && err_cap) snprintf(err, err_cap, "rt_debug_lexicon_compile: bad argument");
    return RT_ERR_INVALID;
  }
  *n_ids_out = 0; *n_entries_out = 0; *n_classes = 0;
  try {
    std::vector<uint8_t> bytes((const uint8_t*)dict, (const uint8_t*)dict + dict_len);
    const std::vector<std::string> d = rt::load_dictionary(bytes);
    *n_classes = (int)d.size();
    std::vector<int32_t> vi, vl;
    rt::compile_lexicon(d, utf8, len, ids, entry_lens, n_id_entries, vi, vl);
    *n_ids_out = (int)vi.size(); *n_entries_out = (int)vl.size();
    if ((size_t)ids_cap < vi.size() || (size_t)lens_cap < vl.size())
      throw RtError(RT_ERR_INVALID, "rt_debug_lexicon_compile: the lexicon needs " + std::to_string(vi.size()) + " ids and " +
                                        std::to_string(vl.size()) + " lengths");
    memcpy(ids_out, vi.data(), vi.size() * sizeof(int32_t));
    memcpy(lens_out, vl.data(), vl.size() * sizeof(int32_t));
    return RT_OK;
  } catch (const RtError& e) {
    if (err && err_cap) snprintf(err, err_cap, "%s", e.what());
    return e.code;
  } catch (const std::exception& e) {
    if (err && err_cap) snprintf(err, err_cap, "%s", e.what());
    return RT_ERR_BACKEND;
  }
}
// both rt_debug_ctc_lexicon*_host forms, arguments already checked; lex_min_post null: the lexicon rule alone
static int lexicon_host(const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line, int n_lines,
                        const int32_t* line_lex, const int32_t* entry_ids, const int32_t* entry_lens, const int32_t* lex_first_entry,
                        int n_lex, float* loglik_out, rt_lexicon_match* matches_out, int32_t* n_matches_out,
                        const float* lex_min_post, int32_t* idx, float* prob, int32_t* snapped_out, float* vit_out) {
  try {
    const int D = 120;
    std::vector<long long> id_off((size_t)lex_first_entry[n_lex] + 1, 0);
    for (int j = 0; j < lex_first_entry[n_lex]; j++) id_off[(size_t)j + 1] = id_off[(size_t)j] + entry_lens[j];
    std::vector<float> logits, lse, row;
    long long o = 0, out = 0;
    for (int i = 0; i < n_lines; i++) {
      const int T = tokens_per_line[i];
      n_matches_out[i] = 0;
      if (line_lex[i] > 0) {
        logits.assign((size_t)std::max(T, 1) * N, 0.0f); lse.assign((size_t)std::max(T, 1), 0.0f);
        for (int t = 0; t < T; t++) {
          cs::row_logits(z5 + (size_t)(o + t) * D, D, W, bias, N, logits.data() + (size_t)t * N);
          lse[(size_t)t] = lx::row_lse(logits.data() + (size_t)t * N, N);
        }
        const int e0 = lex_first_entry[line_lex[i] - 1], n = lex_first_entry[line_lex[i]] - e0;
        row.assign((size_t)n, 0.0f);
        for (int e = 0; e < n; e++)
          row[(size_t)e] = lx::entry_loglik(logits.data(), N, lse.data(), T, entry_ids + id_off[(size_t)(e0 + e)], entry_lens[e0 + e]);
        const lx::Match* m = reinterpret_cast<lx::Match*>(matches_out) + (size_t)i * lx::MATCHES;
        n_matches_out[i] = lx::line_matches(row.data(), n, reinterpret_cast<lx::Match*>(matches_out) + (size_t)i * lx::MATCHES);
        if (loglik_out) memcpy(loglik_out + out, row.data(), (size_t)n * sizeof(float));
        out += n;
        if (lex_min_post) {   // lexicon snap (ctc_lexicon_align.h); m[0] is read only where the line has a match
          const bool fire = la::snaps(lex_min_post[line_lex[i] - 1], n_matches_out[i], n_matches_out[i] >= 1 ? m[0].posterior : 0.0f);
          snapped_out[i] = fire ? 1 : 0;
          if (fire)
            vit_out[i] = la::align_line(logits.data(), N, lse.data(), T, entry_ids + id_off[(size_t)(e0 + m[0].entry)],
                                        entry_lens[e0 + m[0].entry], idx + o, prob + o);
        }
      }
      o += T;
    }
    return RT_OK;
  } catch (const std::exception&) {
    return RT_ERR_BACKEND;
  }
}
int rt_debug_ctc_lexicon_host(const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line,
                              int n_lines, const int32_t* line_lex, const int32_t* entry_ids, const int32_t* entry_lens,
                              const int32_t* lex_first_entry, int n_lex, float* loglik_out, rt_lexicon_match* matches_out,
                              int32_t* n_matches_out) {
  long long rows = 0, table = 0;
  const std::string bad = lexicon_args_error(z5, W, N, tokens_per_line, n_lines, line_lex, entry_ids, entry_lens, lex_first_entry, n_lex,
                                             matches_out, n_matches_out, &rows, &table);
  if (!bad.empty()) {
    rt::create_error() = "rt_debug_ctc_lexicon_host: " + bad;
    return RT_ERR_INVALID;
  }
  return lexicon_host(z5, W, bias, N, tokens_per_line, n_lines, line_lex, entry_ids, entry_lens, lex_first_entry, n_lex, loglik_out,
                      matches_out, n_matches_out, nullptr, nullptr, nullptr, nullptr, nullptr);
}
int rt_debug_ctc_lexicon_align_host(const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line,
                                    int n_lines, const int32_t* line_lex, const int32_t* entry_ids, const int32_t* entry_lens,
                                    const int32_t* lex_first_entry, int n_lex, const float* lex_min_post, int32_t* idx, float* prob,
                                    int32_t* snapped_out, float* vit_out, float* loglik_out, rt_lexicon_match* matches_out,
                                    int32_t* n_matches_out) {
  long long rows = 0, table = 0;
  std::string bad = lexicon_args_error(z5, W, N, tokens_per_line, n_lines, line_lex, entry_ids, entry_lens, lex_first_entry, n_lex,
                                       matches_out, n_matches_out, &rows, &table);
  if (bad.empty()) bad = lexicon_align_args_error(lex_min_post, n_lex, idx, prob, snapped_out, vit_out);
  if (!bad.empty()) {
    rt::create_error() = "rt_debug_ctc_lexicon_align_host: " + bad;
    return RT_ERR_INVALID;
  }
  return lexicon_host(z5, W, bias, N, tokens_per_line, n_lines, line_lex, entry_ids, entry_lens, lex_first_entry, n_lex, loglik_out,
                      matches_out, n_matches_out, lex_min_post, idx, prob, snapped_out, vit_out);
}
static_assert(RT_MAX_KEYWORD_LISTS == kw::MAX_LISTS && RT_KEYWORD_HITS == kw::HITS, "the RT_KEYWORD_* limits and kw:: must agree");
static_assert(sizeof(rt_keyword_hit) == sizeof(kw::Hit) && offsetof(rt_keyword_hit, score) == offsetof(kw::Hit, score) &&
                  offsetof(rt_keyword_hit, first_col) == offsetof(kw::Hit, first_col) && offsetof(rt_keyword_hit, last_col) == offsetof(kw::Hit, last_col) &&
                  offsetof(rt_keyword_hit, quad) == offsetof(kw::Hit, quad), "rt_keyword_hit and kw::Hit must share one layout");
int rt_results_rec_keywords(const rt_results* r, int page, int line, const rt_keyword_hit** hits) {
  auto* p = RT_PAGE(r, page);
  if (!p || line < 0 || (size_t)line >= p->kw_n.size()) return 0;
  if (hits) *hits = reinterpret_cast<const rt_keyword_hit*>(p->kw_hits.data()) + (size_t)line * kw::HITS;
  return p->kw_n[(size_t)line];
}
int rt_results_rec_keywords_id(const rt_results* r, int page, int line) {
  auto* p = RT_PAGE(r, page);
  if (!p || line < 0 || (size_t)line >= p->kw_id.size()) return 0;
  return p->kw_id[(size_t)line];
}
int rt_results_rec_beams(const rt_results* r, int page, int line, const rt_beam** out) {
  auto* p = RT_PAGE(r, page);
  if (!p || p->beam_n <= 0 || line < 0 || (size_t)line >= p->bm_count.size()) return 0;
  if (out) *out = reinterpret_cast<const rt_beam*>(p->bm_recs.data()) + (size_t)line * p->beam_n;
  return p->bm_count[(size_t)line];
}
int rt_results_rec_beam_tokens(const rt_results* r, int page, int line, int k, const int32_t** tokens) {
  auto* p = RT_PAGE(r, page);
  if (!p || p->beam_n <= 0 || line < 0 || (size_t)line >= p->bm_count.size() || k < 0 || k >= p->bm_count[(size_t)line]) return 0;
  const std::vector<int32_t>& t = p->bm_tokens[(size_t)line * p->beam_n + k];
  if (tokens) *tokens = t.data();
  return (int)t.size();
}
const char* rt_results_rec_beam_text(const rt_results* r, int page, int line, int k) {
  auto* p = RT_PAGE(r, page);
  if (!p || p->beam_n <= 0 || line < 0 || (size_t)line >= p->bm_count.size() || k < 0 || k >= p->bm_count[(size_t)line]) return nullptr;
  return p->bm_text[(size_t)line * p->beam_n + k].c_str();
}
int rt_debug_ctc_beam_host(const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line, int n_lines,
                           int beam, int nbest, int32_t* counts_out, rt_beam* beams_out, int32_t* tokens_out) {
  long long rows = 0;
  const std::string bad = beam_args_error(z5, W, N, tokens_per_line, n_lines, beam, nbest, counts_out, beams_out, tokens_out, &rows);
  if (!bad.empty()) {
    rt::create_error() = "rt_debug_ctc_beam_host: " + bad;
    return RT_ERR_INVALID;
  }
  if (beam == 0) return RT_OK;
  try {
    const int D = 120;
    std::vector<float> logits, lse;
    long long o = 0;
    for (int i = 0; i < n_lines; i++) {
      const int T = tokens_per_line[i];
      logits.assign((size_t)std::max(T, 1) * N, 0.0f); lse.assign((size_t)std::max(T, 1), 0.0f);
      for (int t = 0; t < T; t++) {
        cs::row_logits(z5 + (size_t)(o + t) * D, D, W, bias, N, logits.data() + (size_t)t * N);
        lse[(size_t)t] = lx::row_lse(logits.data() + (size_t)t * N, N);
      }
      counts_out[i] = bm::line_beams(logits.data(), N, lse.data(), T, N, beam, nbest, reinterpret_cast<bm::Beam*>(beams_out) + (size_t)i * nbest,
                                     tokens_out + o * nbest);
      o += T;
    }
    return RT_OK;
  } catch (const std::exception&) {
    return RT_ERR_BACKEND;
  }
}
int rt_debug_ctc_keywords_host(const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line, int n_lines,
                               const int32_t* line_kw, const int32_t* entry_ids, const int32_t* entry_lens,
                               const int32_t* kw_first_entry, int n_kw, const float* kw_min_score, float* score_out, int32_t* span_out,
                               rt_keyword_hit* hits_out, int32_t* n_hits_out) {
  long long rows = 0, table = 0;
  const std::string bad = keywords_args_error(z5, W, N, tokens_per_line, n_lines, line_kw, entry_ids, entry_lens, kw_first_entry, n_kw,
                                              kw_min_score, hits_out, n_hits_out, &rows, &table);
  if (!bad.empty()) {
    rt::create_error() = "rt_debug_ctc_keywords_host: " + bad;
    return RT_ERR_INVALID;
  }
  try {
    const int D = 120;
    std::vector<long long> id_off((size_t)kw_first_entry[n_kw] + 1, 0);
    for (int j = 0; j < kw_first_entry[n_kw]; j++) id_off[(size_t)j + 1] = id_off[(size_t)j] + entry_lens[j];
    std::vector<float> logits, rmax, row;
    std::vector<int32_t> span;
    long long o = 0, out = 0;
    for (int i = 0; i < n_lines; i++) {
      const int T = tokens_per_line[i];
      n_hits_out[i] = 0;
      if (line_kw[i] > 0) {
        logits.assign((size_t)std::max(T, 1) * N, 0.0f); rmax.assign((size_t)std::max(T, 1), 0.0f);
        for (int t = 0; t < T; t++) {
          cs::row_logits(z5 + (size_t)(o + t) * D, D, W, bias, N, logits.data() + (size_t)t * N);
          rmax[(size_t)t] = kw::row_max(logits.data() + (size_t)t * N, N);
        }
        const int e0 = kw_first_entry[line_kw[i] - 1], n = kw_first_entry[line_kw[i]] - e0;
        row.assign((size_t)n, 0.0f); span.assign((size_t)2 * n, -1);
        for (int e = 0; e < n; e++)
          row[(size_t)e] = kw::entry_spot(logits.data(), N, rmax.data(), T, entry_ids + id_off[(size_t)(e0 + e)], entry_lens[e0 + e],
                                          span.data() + 2 * (size_t)e);
        n_hits_out[i] = kw::line_hits(row.data(), span.data(), n, kw_min_score[line_kw[i] - 1],
                                      reinterpret_cast<kw::Hit*>(hits_out) + (size_t)i * kw::HITS);
        if (score_out) memcpy(score_out + out, row.data(), (size_t)n * sizeof(float));
        if (span_out) memcpy(span_out + 2 * out, span.data(), (size_t)2 * n * sizeof(int32_t));
        out += n;
      }
      o += T;
    }
    return RT_OK;
  } catch (const std::exception&) {
    return RT_ERR_BACKEND;
  }
}
int rt_debug_span_quad(int T, int W, int resized_w, const float* box8_after, int rot180, int after_w, int after_h, int ori_w, int ori_h,
                       int first_col, int last_col, float* quad8_out) {
  if (!box8_after || !quad8_out || T <= 0 || W <= 0 || resized_w <= 0 || after_w <= 0 || after_h <= 0 || ori_w <= 0 || ori_h <= 0)
    return RT_ERR_INVALID;
  if (first_col < 0 || last_col < first_col || last_col >= T) return RT_ERR_INVALID;
  // the crop as plan_crops (session.cpp) derives it, as rt_debug_word_boxes
  const gm::CropDims cd = gm::crop_dims(box8_after);
  if (cd.w <= 0 || cd.h <= 0) return RT_ERR_IMAGE;
  wb::WordGeom g;
  if (!gm::projection_inverse(box8_after, cd.cw, cd.ch, g.inv)) return RT_ERR_IMAGE;
  g.T = T; g.W = W; g.resized_w = resized_w;
  g.w_c = cd.rot ? cd.h : cd.w; g.h_c = cd.rot ? cd.w : cd.h;
  g.rot270 = cd.rot; g.w = cd.w; g.h = cd.h; g.cw = cd.cw; g.ch = cd.ch;
  kw::span_quad(first_col, last_col, g, rot180 ? 1 : 0, quad8_out);
  gm::scale_and_clip(quad8_out, (double)after_w, (double)after_h, (double)ori_w, (double)ori_h);
  return RT_OK;
}
static_assert(RT_MAX_PATTERNS == pt::MAX_PATTERNS && RT_PATTERN_MAX_STATES == pt::MAX_STATES && RT_PATTERN_MAX_PAIRS == pt::MAX_PAIRS &&
                  RT_PATTERN_MAX_BYTES == pt::MAX_BYTES, "the RT_PATTERN_* limits and pt:: must agree");
static_assert(RT_OK == pt::OK && RT_ERR_UTF8 == pt::ERR_UTF8 && RT_ERR_INVALID == pt::ERR_INVALID && RT_ERR_CAPACITY == pt::ERR_CAPACITY,
              "the status codes of ctc_pattern.h are the RT_ERR_* ones");
int rt_debug_pattern_compile(const void* dict, size_t dict_len, const char* utf8, size_t len, int32_t* group_of_out, int group_cap,
                             int32_t* delta_out, int delta_cap, int32_t* accept_out, int accept_cap, int* S_out, int* G_out, int* P_out,
                             int* min_steps_out, int* n_classes, char* err, size_t err_cap) {
  if (err && err_cap) err[0] = 0;
  if ((!dict && dict_len) || (!utf8 && len) || !S_out || !G_out || !P_out || !min_steps_out || !n_classes || group_cap < 0 ||
      delta_cap < 0 || accept_cap < 0 || (!group_of_out && group_cap) || (!delta_out && delta_cap) || (!accept_out && accept_cap)) {
    if (err && err_cap) snprintf(err, err_cap, "rt_debug_pattern_compile: bad argument");
    return RT_ERR_INVALID;
  }
  *S_out = 0; *G_out = 0; *P_out = 0; *min_steps_out = 0; *n_classes = 0;
  try {
    std::vector<uint8_t> bytes((const uint8_t*)dict, (const uint8_t*)dict + dict_len);
    const std::vector<std::string> d = rt::load_dictionary(bytes);
    *n_classes = (int)d.size();
    pt::Compiled c;
    std::string msg;
    const int rc = pt::compile(d, utf8, len, c, msg);
    if (rc != pt::OK) throw RtError(rc, msg);
    *S_out = c.S; *G_out = c.G; *P_out = c.P; *min_steps_out = c.min_steps;
    if ((size_t)group_cap < c.group_of.size() || (size_t)delta_cap < c.delta.size() || (size_t)accept_cap < c.accept.size())
      throw RtError(RT_ERR_INVALID, "rt_debug_pattern_compile: the pattern needs " + std::to_string(c.group_of.size()) + " groups' ids, " +
                                        std::to_string(c.delta.size()) + " arcs and " + std::to_string(c.accept.size()) + " flags");
    memcpy(group_of_out, c.group_of.data(), c.group_of.size() * sizeof(int32_t));
    memcpy(delta_out, c.delta.data(), c.delta.size() * sizeof(int32_t));
    memcpy(accept_out, c.accept.data(), c.accept.size() * sizeof(int32_t));
    return RT_OK;
  } catch (const RtError& e) {
    if (err && err_cap) snprintf(err, err_cap, "%s", e.what());
    return e.code;
  } catch (const std::exception& e) {
    if (err && err_cap) snprintf(err, err_cap, "%s", e.what());
    return RT_ERR_BACKEND;
  }
}
int rt_debug_ctc_pattern_host(const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line, int n_lines,
                              const int32_t* line_pat, const int32_t* pat_S, const int32_t* pat_G, const int32_t* group_of,
                              const int32_t* delta, const int32_t* accept, int n_pat, int32_t* idx, float* prob, int32_t* matched_out,
                              float* vit_out, float* logprob_out, float* free_out) {
  long long rows = 0;
  std::vector<pt::Rule> rules;
  try {
    const std::string bad = pattern_args_error(z5, W, N, tokens_per_line, n_lines, line_pat, pat_S, pat_G, group_of, delta, accept, n_pat,
                                               idx, prob, matched_out, vit_out, logprob_out, free_out, &rows, &rules);
    if (!bad.empty()) {
      rt::create_error() = "rt_debug_ctc_pattern_host: " + bad;
      return RT_ERR_INVALID;
    }
    const int D = 120;
    std::vector<float> logits, lse;
    long long o = 0;
    for (int i = 0; i < n_lines; i++) {
      const int T = tokens_per_line[i];
      if (line_pat[i] > 0) {
        logits.assign((size_t)std::max(T, 1) * N, 0.0f); lse.assign((size_t)std::max(T, 1), 0.0f);
        for (int t = 0; t < T; t++) {
          cs::row_logits(z5 + (size_t)(o + t) * D, D, W, bias, N, logits.data() + (size_t)t * N);
          lse[(size_t)t] = lx::row_lse(logits.data() + (size_t)t * N, N);
        }
        const pt::LineResult r = pt::viterbi_line(rules[(size_t)line_pat[i] - 1], logits.data(), N, lse.data(), T, idx + o, prob + o);
        matched_out[i] = r.matched; vit_out[i] = r.vit; logprob_out[i] = r.logprob; free_out[i] = r.free_logprob;
      }
      o += T;
    }
    return RT_OK;
  } catch (const std::exception&) {
    return RT_ERR_BACKEND;
  }
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
    s->prof.clear(); s->prof.on = mode;
    for (auto& h : s->helpers) { h->prof.clear(); h->prof.on = mode; }
  });
}
int rt_profile_get(rt_session* s, const char* const** names, const float** ms, const int** calls, int* n) {
  RT_REQUIRE(s && names && ms && calls && n, s, "rt_profile_get: null argument");
  for (auto& h : s->helpers) s->prof.merge(h->prof);
  *names = s->prof.names.data(); *ms = s->prof.ms.data(); *calls = s->prof.calls.data(); *n = (int)s->prof.names.size();
  return RT_OK;
}

int rt_onnx_to_rtwb(int which, const void* onnx, size_t len, void** out, size_t* out_len, char* err, size_t err_cap) {
  if (err && err_cap) err[0] = 0;
  if (!onnx || !len || !out || !out_len) { if (err && err_cap) snprintf(err, err_cap, "rt_onnx_to_rtwb: null argument"); return RT_ERR_INVALID; }
  try {
    std::vector<uint8_t> b = rt::onnx_to_rtwb(which, (const uint8_t*)onnx, len);
    void* p = malloc(b.size());
    if (!p) throw RtError(RT_ERR_BACKEND, "out of memory");
    memcpy(p, b.data(), b.size());
    *out = p; *out_len = b.size();
    return RT_OK;
  } catch (const RtError& e) {
    if (err && err_cap) snprintf(err, err_cap, "%s", e.what());
    return e.code;
  } catch (const std::exception& e) {
    if (err && err_cap) snprintf(err, err_cap, "%s", e.what());
    return RT_ERR_BACKEND;
  }
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
