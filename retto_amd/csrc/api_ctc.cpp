// The debug entries of the rec CTC tail's options (include/retto_hip.h), both forms of each next to each other: rt_debug_ctc_*_host
// runs the host reference of ctc_host_ref.h, rt_debug_ctc_* runs the same call through rt_session::rec_tail on the device
// (TailHook), and the rt_debug_*_compile hooks compile a charset, a lexicon or a pattern without a session.  An entry fills its
// kind's argument struct (ctc_host_ref.h) by name, checks it, puts its own name before the message, and runs the reference or the hook.
#include <cstdio>
#include <cstring>
#include <numeric>

#include "api_internal.h"
#include "ctc_host_ref.h"

using namespace rt;

static_assert(sizeof(rt_candidate) == sizeof(cc::Cand) && offsetof(rt_candidate, prob) == offsetof(cc::Cand, prob) &&
                  RT_MAX_CANDIDATES == cc::MAX_K, "rt_candidate and cc::Cand must share one layout");
static_assert(RT_MAX_CHARSETS == cs::MAX_SETS, "RT_MAX_CHARSETS and cs::MAX_SETS must agree");
static_assert(RT_MAX_LEXICONS == lx::MAX_LEXICONS && RT_LEXICON_MAX_ENTRIES == lx::MAX_ENTRIES && RT_LEXICON_MAX_LEN == lx::MAX_LEN &&
                  RT_LEXICON_MATCHES == lx::MATCHES, "the RT_LEXICON_* limits and lx:: must agree");
static_assert(sizeof(rt_lexicon_match) == sizeof(lx::Match) && offsetof(rt_lexicon_match, loglik) == offsetof(lx::Match, loglik) &&
                  offsetof(rt_lexicon_match, posterior) == offsetof(lx::Match, posterior), "rt_lexicon_match and lx::Match must share one layout");
static_assert(RT_MAX_KEYWORD_LISTS == kw::MAX_LISTS && RT_KEYWORD_HITS == kw::HITS, "the RT_KEYWORD_* limits and kw:: must agree");
static_assert(sizeof(rt_keyword_hit) == sizeof(kw::Hit) && offsetof(rt_keyword_hit, score) == offsetof(kw::Hit, score) &&
                  offsetof(rt_keyword_hit, first_col) == offsetof(kw::Hit, first_col) && offsetof(rt_keyword_hit, last_col) == offsetof(kw::Hit, last_col) &&
                  offsetof(rt_keyword_hit, quad) == offsetof(kw::Hit, quad), "rt_keyword_hit and kw::Hit must share one layout");
static_assert(RT_MAX_BEAM == bm::MAX_BEAM && RT_MAX_NBEST == bm::MAX_NBEST, "the RT_MAX_BEAM / RT_MAX_NBEST limits and bm:: must agree");
static_assert(sizeof(rt_beam) == sizeof(bm::Beam) && offsetof(rt_beam, logprob) == offsetof(bm::Beam, logprob) &&
                  offsetof(rt_beam, n_tokens) == offsetof(bm::Beam, n_tokens), "rt_beam and bm::Beam must share one layout");
static_assert(RT_MAX_LM_ORDER == lm::MAX_ORDER && RT_MAX_LM_NGRAMS == lm::MAX_NGRAMS && RT_MAX_LMS == lm::MAX_LMS, "the RT_MAX_LM* limits and lm:: must agree");
static_assert(sizeof(rt_beam_lm) == sizeof(lm::BeamLm) && offsetof(rt_beam_lm, lm) == offsetof(lm::BeamLm, lm) &&
                  offsetof(rt_beam_lm, score) == offsetof(lm::BeamLm, score), "rt_beam_lm and lm::BeamLm must share one layout");
static_assert(RT_OK == lm::OK && RT_ERR_INVALID == lm::ERR_INVALID, "the status codes of ctc_lm.h are the RT_ERR_* ones");
static_assert(RT_VOCAB_MAX_LEN == vc::MAX_LEN && RT_VOCAB_MAX_WORDS == vc::MAX_WORDS && RT_MAX_VOCABS == vc::MAX_VOCABS &&
                  RT_VOCAB_CASE_VARIANTS == vc::CASE_VARIANTS, "the RT_VOCAB_* limits and vc:: must agree");
static_assert(sizeof(rt_beam_vocab) == sizeof(vc::BeamVocab) && offsetof(rt_beam_vocab, oov_words) == offsetof(vc::BeamVocab, oov_words) &&
                  offsetof(rt_beam_vocab, score) == offsetof(vc::BeamVocab, score), "rt_beam_vocab and vc::BeamVocab must share one layout");
static_assert(RT_OK == vc::OK && RT_ERR_INVALID == vc::ERR_INVALID && RT_ERR_CAPACITY == vc::ERR_CAPACITY, "the status codes of ctc_vocab.h are the RT_ERR_* ones");
static_assert(RT_MAX_PATTERNS == pt::MAX_PATTERNS && RT_PATTERN_MAX_STATES == pt::MAX_STATES && RT_PATTERN_MAX_PAIRS == pt::MAX_PAIRS &&
                  RT_PATTERN_MAX_BYTES == pt::MAX_BYTES, "the RT_PATTERN_* limits and pt:: must agree");
static_assert(RT_OK == pt::OK && RT_ERR_UTF8 == pt::ERR_UTF8 && RT_ERR_INVALID == pt::ERR_INVALID && RT_ERR_CAPACITY == pt::ERR_CAPACITY,
              "the status codes of ctc_pattern.h are the RT_ERR_* ones");

namespace {

// The host form of an entry whose check speaks: the first failed requirement under the entry's name (rt_last_error(NULL)), else
// the reference.  (The check runs inside the guard: a pattern's builds its rules.)
template <class A>
int host_entry(const char* name, A& a, void (*ref)(const A&)) {
  try {
    const std::string bad = a.error();
    if (!bad.empty()) {
      create_error() = std::string(name) + ": " + bad;
      return RT_ERR_INVALID;
    }
    ref(a);
    return RT_OK;
  } catch (const std::exception&) { return RT_ERR_BACKEND; }
}
// ... and of one whose check only answers yes or no (candidates, charsets), already made
template <class A>
int host_run(const A& a, void (*ref)(const A&)) {
  try {
    ref(a);
    return RT_OK;
  } catch (const std::exception&) { return RT_ERR_BACKEND; }
}
// What the device form of such an entry requires before any device work, in this order: a session, the struct's check, chunk_rows.
template <class A>
int device_check(rt_session* s, const std::string& name, A& a, int chunk_rows) {
  RT_REQUIRE(s, s, name + ": null session");
  const std::string bad = a.error();
  RT_REQUIRE(bad.empty(), s, name + ": " + bad);
  RT_REQUIRE(chunk_rows >= 0, s, name + ": chunk_rows is negative");
  return RT_OK;
}

// What a call adds to its Head for the tail: the decoded rows (null: zeros, the decode's results are then thrown away), the
// candidates' K, the row chunk of the line passes, and -- beam_b > 0 -- the beam every line carries.
struct TailIn { const int32_t* idx = nullptr; const float* prob = nullptr; int K = 0, chunk_rows = 0, beam_b = 0, beam_n = 0; };
// One rec group on host arrays through rt_session::rec_tail, the tail rec_groups runs per group, on the plan of rec_tail_plan.h
// over the caller's lines: the features inside a larger zeroed allocation, as z5 sits inside the scratch arena; an FC packed by
// pack_linear; the lines' geometry as the token level gives it; opts: the lines' options (lines_with), whose ids count into
// `stores`.  An entry adds its own kind's tables, inputs and outputs to `t`, run()s, and downloads.
struct TailHook {
  rt_session* s; size_t nr;
  WeightStore ws; SvtrCore core; DevBufs bufs;
  RecTailPlan plan; rt_session::RecTail t;
  TailHook(rt_session* s_, const hr::Head& a, const TailIn& in, const std::vector<RecLineOpts>& opts, const RecStores& stores)
      : s(s_), nr((size_t)std::max<long long>(a.rows, 1)) {
    if (core.D != hr::HEAD_D) throw RtError(RT_ERR_BACKEND, "the CTC head's input width is not the host references' (hr::HEAD_D)");
    s->begin_call();
    const int n_lines = a.n_lines;
    std::vector<long long> off((size_t)n_lines + 1, 0);
    std::partial_sum(a.tokens_per_line, a.tokens_per_line + n_lines, off.begin() + 1);   // (below 2^30: the entries' own check)
    plan = rec_tail_plan(off.data(), 0, n_lines, opts.data(), stores, in.beam_b, in.beam_n);
    t.beam.b = in.beam_b; t.beam.n = in.beam_n;
    core.classes = a.N;
    if (plan.needs_z5(in.K)) {
      core.fc = pack_linear(ws, a.W, a.bias, core.D, a.N);
      float* dz = bufs.zeroed<float>((nr + 256) * core.D);
      DevBufs::put(dz, a.z5, (size_t)a.rows * core.D); t.z5 = dz;
    }
    const std::vector<int32_t> zeros(in.idx ? 0 : nr, 0);
    t.idx = bufs.upload(in.idx ? in.idx : zeros.data(), in.idx ? (size_t)a.rows : nr);
    t.prob = bufs.upload(in.prob ? in.prob : reinterpret_cast<const float*>(zeros.data()), in.prob ? (size_t)a.rows : nr);
    t.lines = Ragged(a.tokens_per_line, n_lines).upload(bufs); t.n_lines = n_lines;
    t.tok = bufs.alloc<int>(nr); t.ntok = bufs.alloc<int>(n_lines); t.rscore = bufs.alloc<float>(n_lines);
    t.cand.k = in.K; t.chunk_rows = in.chunk_rows;
  }
  // rec_return_candidates: what the kernels write starts as the caller's values
  void candidates(const int32_t* cols, const rt_candidate* cands) {
    t.cand.col = bufs.alloc<int>(nr); t.cand.cands = bufs.alloc<cc::Cand>(nr * t.cand.k); DevBufs::put(t.cand.col, cols, (size_t)plan.rows);
    DevBufs::put(t.cand.cands, reinterpret_cast<const cc::Cand*>(cands), (size_t)plan.rows * t.cand.k);
  }
  void run() { s->rec_tail(plan, core, t); RT_HIP_CHECK(hipStreamSynchronize(s->st)); }
  void download_candidates(int32_t* cols, rt_candidate* cands) const {
    DevBufs::download(cols, t.cand.col, (size_t)plan.rows);
    DevBufs::download(reinterpret_cast<cc::Cand*>(cands), t.cand.cands, (size_t)plan.rows * t.cand.k);
  }
};
// the lists of a lexicon or keyword entry as lx::Tables, built as rt_lexicon_create / rt_keywords_create build them
lx::Tables tables_of(const hr::EntryLists& e) {
  lx::Tables tb;
  long long io = 0;
  for (int k = 0; k < e.n; k++) {
    const int e0 = e.first_entry[k], n = e.first_entry[k + 1] - e0;
    tb.add(e.entry_ids + io, e.entry_lens + e0, n);
    for (int j = 0; j < n; j++) io += e.entry_lens[e0 + j];
  }
  return tb;
}

// Rec lexicons' device path on host arrays.  With a.align (lexicon snap, ctc_lexicon_align.h) also the caller's idx / prob rows,
// in and out, the flags and the Viterbi values; a threshold above 0 on the lexicon of some line makes the group a snap group.
void debug_ctc_lexicon(rt_session* s, const hr::LexiconArgs& a, int chunk_rows) {
  const int n_lines = a.n_lines;
  const lx::Tables tb = tables_of(a.lists);
  TailHook h(s, a, {a.idx, a.prob, 0, chunk_rows}, lines_with(n_lines, &RecLineOpts::lexicon, a.line_lex), RecStores{&tb, a.lex_min_post});
  rt_entry_store X;   // (the tables on the device, freed on every way out)
  X.set(tb);
  for (int i = 0; i < n_lines; i++) {   // (a line without a lexicon has no match; the kernel, where it runs, writes every lexicon line's flag again)
    if (a.line_lex[i] <= 0) a.n_matches_out[i] = 0;
    else if (a.align) a.snapped_out[i] = 0;
  }
  rt_session::RecTail::Lexicon& t = h.t.lexicon;
  t.d = X.d;
  // (what the kernels write starts as the caller's values: a slot they leave alone comes back untouched)
  t.loglik = h.bufs.alloc<float>((size_t)h.plan.table);
  if (a.loglik_out) DevBufs::put(t.loglik, a.loglik_out, (size_t)h.plan.table);
  t.matches = h.bufs.upload(reinterpret_cast<const lx::Match*>(a.matches_out), (size_t)n_lines * lx::MATCHES);
  t.n = h.bufs.upload(a.n_matches_out, (size_t)n_lines);
  if (a.align) {
    t.d_min_post = h.bufs.upload(a.lex_min_post, (size_t)a.lists.n);
    t.snapped = h.bufs.upload(a.snapped_out, (size_t)n_lines); t.vit = h.bufs.upload(a.vit_out, (size_t)n_lines);
  }
  h.run();
  if (a.loglik_out) DevBufs::download(a.loglik_out, t.loglik, (size_t)h.plan.table);
  DevBufs::download(reinterpret_cast<lx::Match*>(a.matches_out), t.matches, (size_t)n_lines * lx::MATCHES);
  DevBufs::download(a.n_matches_out, t.n, (size_t)n_lines);
  if (a.align) {
    DevBufs::download(a.idx, h.t.idx, (size_t)a.rows); DevBufs::download(a.prob, h.t.prob, (size_t)a.rows);
    DevBufs::download(a.snapped_out, t.snapped, (size_t)n_lines); DevBufs::download(a.vit_out, t.vit, (size_t)n_lines);
  }
}

// What the three rt_debug_*_compile hooks share: err cleared, `bad` (the entry's own argument check) refused under its name,
// the dictionary parsed and counted into *n_classes, then body(dictionary); an RtError's code comes back, its message in err.
template <class F>
int compile_hook(const char* name, bool bad, const void* dict, size_t dict_len, int* n_classes, char* err, size_t err_cap, F&& body) {
  if (err && err_cap) err[0] = 0;
  if (bad) {
    if (err && err_cap) snprintf(err, err_cap, "%s: bad argument", name);
    return RT_ERR_INVALID;
  }
  *n_classes = 0;
  try {
    const std::vector<uint8_t> bytes((const uint8_t*)dict, (const uint8_t*)dict + dict_len);
    const std::vector<std::string> d = rt::load_dictionary(bytes);
    *n_classes = (int)d.size();
    body(d);
    return RT_OK;
  } catch (const RtError& e) {
    if (err && err_cap) snprintf(err, err_cap, "%s", e.what());
    return e.code;
  } catch (const std::exception& e) {
    if (err && err_cap) snprintf(err, err_cap, "%s", e.what());
    return RT_ERR_BACKEND;
  }
}

}  // namespace

extern "C" {

// ---- candidates: rt_config.rec_return_candidates' path on host arrays (pp::ctc_decode for the token counts, then the candidates)
int rt_debug_ctc_candidates_host(const float* z5, const float* W, const float* bias, int N, const int32_t* idx, const float* prob,
                                 const int32_t* tokens_per_line, int n_lines, int K, rt_candidate* cands_out, int32_t* cols_out,
                                 int32_t* n_tokens_out) {
  hr::CandArgs a{{z5, W, bias, N, tokens_per_line, n_lines}};
  a.idx = idx; a.prob = prob; a.K = K; a.cands_out = cands_out; a.cols_out = cols_out; a.n_tokens_out = n_tokens_out;
  if (!a.ok()) return RT_ERR_INVALID;
  return host_run(a, hr::candidates_ref);
}
RT_API int rt_debug_ctc_candidates(rt_session* s, const float* z5, const float* W, const float* bias, int N, const int32_t* idx,
                                   const float* prob, const int32_t* tokens_per_line, int n_lines, int K, int chunk_rows,
                                   rt_candidate* cands_out, int32_t* cols_out, int32_t* n_tokens_out) {
  hr::CandArgs a{{z5, W, bias, N, tokens_per_line, n_lines}};
  a.idx = idx; a.prob = prob; a.K = K; a.cands_out = cands_out; a.cols_out = cols_out; a.n_tokens_out = n_tokens_out;
  RT_REQUIRE(s, s, "rt_debug_ctc_candidates: null session");
  RT_REQUIRE(a.ok() && chunk_rows >= 0, s, "rt_debug_ctc_candidates: bad argument");
  return guarded(s, [&] {
    TailHook h(s, a, {idx, prob, K, chunk_rows}, std::vector<RecLineOpts>((size_t)n_lines), RecStores{});
    h.candidates(cols_out, cands_out);
    h.run();
    DevBufs::download(n_tokens_out, h.t.ntok, (size_t)n_lines);
    h.download_candidates(cols_out, cands_out);
  });
}

// ---- charsets: the restricted rows' argmax, the decode and -- K > 0 -- the candidates with the masks
int rt_debug_charset_compile(const void* dict, size_t dict_len, const char* utf8, size_t len, const int32_t* ids, int n_ids,
                             uint32_t* mask_out, int mask_cap, int* n_classes, char* err, size_t err_cap) {
  const bool bad = (!dict && dict_len) || (!utf8 && len) || n_ids < 0 || (!ids && n_ids) || !n_classes || mask_cap < 0 || (!mask_out && mask_cap);
  return compile_hook("rt_debug_charset_compile", bad, dict, dict_len, n_classes, err, err_cap, [&](const std::vector<std::string>& d) {
    const std::vector<uint32_t> mask = rt::compile_charset(d, utf8, len, ids, n_ids);
    if ((size_t)mask_cap < mask.size()) throw RtError(RT_ERR_INVALID, "rt_debug_charset_compile: the mask needs " + std::to_string(mask.size()) + " words");
    memcpy(mask_out, mask.data(), mask.size() * sizeof(uint32_t));
  });
}
int rt_debug_ctc_charset_host(const float* z5, const float* W, const float* bias, int N, int32_t* idx, float* prob,
                              const int32_t* tokens_per_line, int n_lines, const int32_t* line_set, const uint32_t* masks,
                              int n_sets, int K, int32_t* tokens_out, int32_t* n_tokens_out, float* scores_out,
                              rt_candidate* cands_out, int32_t* cols_out) {
  hr::CharsetArgs a{{z5, W, bias, N, tokens_per_line, n_lines}};
  a.idx = idx; a.prob = prob; a.line_set = line_set; a.masks = masks; a.n_sets = n_sets; a.K = K;
  a.tokens_out = tokens_out; a.n_tokens_out = n_tokens_out; a.scores_out = scores_out; a.cands_out = cands_out; a.cols_out = cols_out;
  if (!a.ok()) return RT_ERR_INVALID;
  return host_run(a, hr::charset_ref);
}
RT_API int rt_debug_ctc_charset(rt_session* s, const float* z5, const float* W, const float* bias, int N, int32_t* idx, float* prob,
                                const int32_t* tokens_per_line, int n_lines, const int32_t* line_set, const uint32_t* masks,
                                int n_sets, int K, int chunk_rows, int32_t* tokens_out, int32_t* n_tokens_out, float* scores_out,
                                rt_candidate* cands_out, int32_t* cols_out) {
  hr::CharsetArgs a{{z5, W, bias, N, tokens_per_line, n_lines}};
  a.idx = idx; a.prob = prob; a.line_set = line_set; a.masks = masks; a.n_sets = n_sets; a.K = K;
  a.tokens_out = tokens_out; a.n_tokens_out = n_tokens_out; a.scores_out = scores_out; a.cands_out = cands_out; a.cols_out = cols_out;
  RT_REQUIRE(s, s, "rt_debug_ctc_charset: null session");
  RT_REQUIRE(a.ok() && chunk_rows >= 0, s, "rt_debug_ctc_charset: bad argument");
  return guarded(s, [&] {
    TailHook h(s, a, {idx, prob, K, chunk_rows}, lines_with(n_lines, &RecLineOpts::charset, line_set), RecStores{});
    h.t.charsets.words = cs::mask_words(N);
    h.t.charsets.masks = n_sets > 0 ? h.bufs.upload(masks, (size_t)n_sets * h.t.charsets.words) : nullptr;
    DevBufs::put(h.t.tok, tokens_out, (size_t)a.rows);
    if (K > 0) h.candidates(cols_out, cands_out);
    h.run();
    DevBufs::download(idx, h.t.idx, (size_t)a.rows); DevBufs::download(prob, h.t.prob, (size_t)a.rows);
    DevBufs::download(tokens_out, h.t.tok, (size_t)a.rows);
    DevBufs::download(n_tokens_out, h.t.ntok, (size_t)n_lines); DevBufs::download(scores_out, h.t.rscore, (size_t)n_lines);
    if (K > 0) h.download_candidates(cols_out, cands_out);
  });
}

// ---- lexicons, and lexicon snap (the _align forms)
int rt_debug_lexicon_compile(const void* dict, size_t dict_len, const char* utf8, size_t len, const int32_t* ids,
                             const int32_t* entry_lens, int n_id_entries, int32_t* ids_out, int ids_cap, int32_t* lens_out,
                             int lens_cap, int* n_ids_out, int* n_entries_out, int* n_classes, char* err, size_t err_cap) {
  const bool bad = (!dict && dict_len) || (!utf8 && len) || n_id_entries < 0 || ((!ids || !entry_lens) && n_id_entries) || !n_ids_out ||
                   !n_entries_out || !n_classes || ids_cap < 0 || lens_cap < 0 || (!ids_out && ids_cap) || (!lens_out && lens_cap);
  if (!bad) { *n_ids_out = 0; *n_entries_out = 0; }
  return compile_hook("rt_debug_lexicon_compile", bad, dict, dict_len, n_classes, err, err_cap, [&](const std::vector<std::string>& d) {
    std::vector<int32_t> vi, vl;
    rt::compile_lexicon(d, utf8, len, ids, entry_lens, n_id_entries, vi, vl);
    *n_ids_out = (int)vi.size(); *n_entries_out = (int)vl.size();
    if ((size_t)ids_cap < vi.size() || (size_t)lens_cap < vl.size())
      throw RtError(RT_ERR_INVALID, "rt_debug_lexicon_compile: the lexicon needs " + std::to_string(vi.size()) + " ids and " +
                                        std::to_string(vl.size()) + " lengths");
    memcpy(ids_out, vi.data(), vi.size() * sizeof(int32_t));
    memcpy(lens_out, vl.data(), vl.size() * sizeof(int32_t));
  });
}
int rt_debug_ctc_lexicon_host(const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line,
                              int n_lines, const int32_t* line_lex, const int32_t* entry_ids, const int32_t* entry_lens,
                              const int32_t* lex_first_entry, int n_lex, float* loglik_out, rt_lexicon_match* matches_out,
                              int32_t* n_matches_out) {
  hr::LexiconArgs a{{z5, W, bias, N, tokens_per_line, n_lines}};
  a.line_lex = line_lex; a.lists = {entry_ids, entry_lens, lex_first_entry, n_lex};
  a.loglik_out = loglik_out; a.matches_out = matches_out; a.n_matches_out = n_matches_out;
  return host_entry("rt_debug_ctc_lexicon_host", a, hr::lexicon_ref);
}
RT_API int rt_debug_ctc_lexicon(rt_session* s, const float* z5, const float* W, const float* bias, int N,
                                const int32_t* tokens_per_line, int n_lines, const int32_t* line_lex, const int32_t* entry_ids,
                                const int32_t* entry_lens, const int32_t* lex_first_entry, int n_lex, int chunk_rows,
                                float* loglik_out, rt_lexicon_match* matches_out, int32_t* n_matches_out) {
  hr::LexiconArgs a{{z5, W, bias, N, tokens_per_line, n_lines}};
  a.line_lex = line_lex; a.lists = {entry_ids, entry_lens, lex_first_entry, n_lex};
  a.loglik_out = loglik_out; a.matches_out = matches_out; a.n_matches_out = n_matches_out;
  if (const int rc = device_check(s, "rt_debug_ctc_lexicon", a, chunk_rows)) return rc;
  return guarded(s, [&] { debug_ctc_lexicon(s, a, chunk_rows); });
}
int rt_debug_ctc_lexicon_align_host(const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line,
                                    int n_lines, const int32_t* line_lex, const int32_t* entry_ids, const int32_t* entry_lens,
                                    const int32_t* lex_first_entry, int n_lex, const float* lex_min_post, int32_t* idx, float* prob,
                                    int32_t* snapped_out, float* vit_out, float* loglik_out, rt_lexicon_match* matches_out,
                                    int32_t* n_matches_out) {
  hr::LexiconArgs a{{z5, W, bias, N, tokens_per_line, n_lines}};
  a.line_lex = line_lex; a.lists = {entry_ids, entry_lens, lex_first_entry, n_lex};
  a.loglik_out = loglik_out; a.matches_out = matches_out; a.n_matches_out = n_matches_out;
  a.align = true; a.lex_min_post = lex_min_post; a.idx = idx; a.prob = prob; a.snapped_out = snapped_out; a.vit_out = vit_out;
  return host_entry("rt_debug_ctc_lexicon_align_host", a, hr::lexicon_ref);
}
RT_API int rt_debug_ctc_lexicon_align(rt_session* s, const float* z5, const float* W, const float* bias, int N,
                                      const int32_t* tokens_per_line, int n_lines, const int32_t* line_lex, const int32_t* entry_ids,
                                      const int32_t* entry_lens, const int32_t* lex_first_entry, int n_lex, const float* lex_min_post,
                                      int chunk_rows, int32_t* idx, float* prob, int32_t* snapped_out, float* vit_out,
                                      float* loglik_out, rt_lexicon_match* matches_out, int32_t* n_matches_out) {
  hr::LexiconArgs a{{z5, W, bias, N, tokens_per_line, n_lines}};
  a.line_lex = line_lex; a.lists = {entry_ids, entry_lens, lex_first_entry, n_lex};
  a.loglik_out = loglik_out; a.matches_out = matches_out; a.n_matches_out = n_matches_out;
  a.align = true; a.lex_min_post = lex_min_post; a.idx = idx; a.prob = prob; a.snapped_out = snapped_out; a.vit_out = vit_out;
  if (const int rc = device_check(s, "rt_debug_ctc_lexicon_align", a, chunk_rows)) return rc;
  return guarded(s, [&] { debug_ctc_lexicon(s, a, chunk_rows); });
}

// ---- patterns; the device form builds the pattern tables as a session's store would (pt::Rule::build from the flat compiled
// tables, pt::Tables)
int rt_debug_pattern_compile(const void* dict, size_t dict_len, const char* utf8, size_t len, int32_t* group_of_out, int group_cap,
                             int32_t* delta_out, int delta_cap, int32_t* accept_out, int accept_cap, int* S_out, int* G_out, int* P_out,
                             int* min_steps_out, int* n_classes, char* err, size_t err_cap) {
  const bool bad = (!dict && dict_len) || (!utf8 && len) || !S_out || !G_out || !P_out || !min_steps_out || !n_classes || group_cap < 0 ||
                   delta_cap < 0 || accept_cap < 0 || (!group_of_out && group_cap) || (!delta_out && delta_cap) || (!accept_out && accept_cap);
  if (!bad) { *S_out = 0; *G_out = 0; *P_out = 0; *min_steps_out = 0; }
  return compile_hook("rt_debug_pattern_compile", bad, dict, dict_len, n_classes, err, err_cap, [&](const std::vector<std::string>& d) {
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
  });
}
int rt_debug_ctc_pattern_host(const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line, int n_lines,
                              const int32_t* line_pat, const int32_t* pat_S, const int32_t* pat_G, const int32_t* group_of,
                              const int32_t* delta, const int32_t* accept, int n_pat, int32_t* idx, float* prob, int32_t* matched_out,
                              float* vit_out, float* logprob_out, float* free_out) {
  hr::PatternArgs a{{z5, W, bias, N, tokens_per_line, n_lines}};
  a.line_pat = line_pat; a.pat_S = pat_S; a.pat_G = pat_G; a.group_of = group_of; a.delta = delta; a.accept = accept; a.n_pat = n_pat;
  a.idx = idx; a.prob = prob; a.matched_out = matched_out; a.vit_out = vit_out; a.logprob_out = logprob_out; a.free_out = free_out;
  return host_entry("rt_debug_ctc_pattern_host", a, hr::pattern_ref);
}
RT_API int rt_debug_ctc_pattern(rt_session* s, const float* z5, const float* W, const float* bias, int N,
                                const int32_t* tokens_per_line, int n_lines, const int32_t* line_pat, const int32_t* pat_S,
                                const int32_t* pat_G, const int32_t* group_of, const int32_t* delta, const int32_t* accept, int n_pat,
                                int chunk_rows, int32_t* idx, float* prob, int32_t* matched_out, float* vit_out, float* logprob_out,
                                float* free_out) {
  hr::PatternArgs a{{z5, W, bias, N, tokens_per_line, n_lines}};
  a.line_pat = line_pat; a.pat_S = pat_S; a.pat_G = pat_G; a.group_of = group_of; a.delta = delta; a.accept = accept; a.n_pat = n_pat;
  a.idx = idx; a.prob = prob; a.matched_out = matched_out; a.vit_out = vit_out; a.logprob_out = logprob_out; a.free_out = free_out;
  if (const int rc = device_check(s, "rt_debug_ctc_pattern", a, chunk_rows)) return rc;
  return guarded(s, [&] {
    pt::Tables tb;
    for (const pt::Rule& r : a.rules) tb.add(r);
    TailHook h(s, a, {idx, prob, 0, chunk_rows}, lines_with(n_lines, &RecLineOpts::pattern, line_pat), RecStores{nullptr, nullptr, &tb});
    rt_session::RecTail::Pattern& t = h.t.pattern;
    t.d = pt::DevTables{h.bufs.upload(tb.pats.data(), tb.pats.size()), h.bufs.upload(tb.pair_c.data(), tb.pair_c.size()),
                        h.bufs.upload(tb.pair_pb.data(), tb.pair_pb.size()), h.bufs.upload(tb.pair_pe.data(), tb.pair_pe.size()),
                        h.bufs.upload(tb.seg.data(), tb.seg.size()), h.bufs.upload(tb.preds.data(), tb.preds.size())};
    // (what the kernel writes starts as the caller's values: a slot it leaves alone comes back untouched)
    t.matched = h.bufs.upload(matched_out, (size_t)n_lines); t.vit = h.bufs.upload(vit_out, (size_t)n_lines);
    t.logprob = h.bufs.upload(logprob_out, (size_t)n_lines); t.free_logprob = h.bufs.upload(free_out, (size_t)n_lines);
    h.run();
    DevBufs::download(idx, h.t.idx, (size_t)a.rows); DevBufs::download(prob, h.t.prob, (size_t)a.rows);
    DevBufs::download(matched_out, t.matched, (size_t)n_lines); DevBufs::download(vit_out, t.vit, (size_t)n_lines);
    DevBufs::download(logprob_out, t.logprob, (size_t)n_lines); DevBufs::download(free_out, t.free_logprob, (size_t)n_lines);
  });
}

// ---- keywords; the device form builds the list tables as rt_keywords_create builds them (lx::Tables)
int rt_debug_ctc_keywords_host(const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line, int n_lines,
                               const int32_t* line_kw, const int32_t* entry_ids, const int32_t* entry_lens,
                               const int32_t* kw_first_entry, int n_kw, const float* kw_min_score, float* score_out, int32_t* span_out,
                               rt_keyword_hit* hits_out, int32_t* n_hits_out) {
  hr::KeywordArgs a{{z5, W, bias, N, tokens_per_line, n_lines}};
  a.line_kw = line_kw; a.lists = {entry_ids, entry_lens, kw_first_entry, n_kw}; a.kw_min_score = kw_min_score;
  a.score_out = score_out; a.span_out = span_out; a.hits_out = hits_out; a.n_hits_out = n_hits_out;
  return host_entry("rt_debug_ctc_keywords_host", a, hr::keywords_ref);
}
RT_API int rt_debug_ctc_keywords(rt_session* s, const float* z5, const float* W, const float* bias, int N,
                                 const int32_t* tokens_per_line, int n_lines, const int32_t* line_kw, const int32_t* entry_ids,
                                 const int32_t* entry_lens, const int32_t* kw_first_entry, int n_kw, const float* kw_min_score,
                                 int chunk_rows, float* score_out, int32_t* span_out, rt_keyword_hit* hits_out, int32_t* n_hits_out) {
  hr::KeywordArgs a{{z5, W, bias, N, tokens_per_line, n_lines}};
  a.line_kw = line_kw; a.lists = {entry_ids, entry_lens, kw_first_entry, n_kw}; a.kw_min_score = kw_min_score;
  a.score_out = score_out; a.span_out = span_out; a.hits_out = hits_out; a.n_hits_out = n_hits_out;
  if (const int rc = device_check(s, "rt_debug_ctc_keywords", a, chunk_rows)) return rc;
  return guarded(s, [&] {
    const lx::Tables tb = tables_of(a.lists);
    TailHook h(s, a, {nullptr, nullptr, 0, chunk_rows}, lines_with(n_lines, &RecLineOpts::keywords, line_kw), RecStores{nullptr, nullptr, nullptr, &tb});
    rt_entry_store X;   // (the tables on the device, freed on every way out)
    X.set(tb);
    for (int i = 0; i < n_lines; i++)   // (a line without a list has no hit)
      if (line_kw[i] <= 0) n_hits_out[i] = 0;
    rt_session::RecTail::Keywords& t = h.t.keywords;
    t.d = X.d;
    t.d_min = h.bufs.upload(kw_min_score, (size_t)n_kw);
    // (what the kernels write starts as the caller's values: a slot they leave alone comes back untouched)
    const size_t tn = (size_t)std::max<long long>(a.table, 1);
    t.score = h.bufs.alloc<float>(tn); t.span = h.bufs.alloc<int>(2 * tn);
    if (score_out) DevBufs::put(t.score, score_out, (size_t)a.table);
    if (span_out) DevBufs::put(t.span, span_out, 2 * (size_t)a.table);
    t.hits = h.bufs.upload(reinterpret_cast<const kw::Hit*>(hits_out), (size_t)n_lines * kw::HITS);
    t.n = h.bufs.upload(n_hits_out, (size_t)n_lines);
    h.run();
    if (score_out) DevBufs::download(score_out, t.score, (size_t)a.table);
    if (span_out) DevBufs::download(span_out, t.span, 2 * (size_t)a.table);
    DevBufs::download(reinterpret_cast<kw::Hit*>(hits_out), t.hits, (size_t)n_lines * kw::HITS);
    DevBufs::download(n_hits_out, t.n, (size_t)n_lines);
  });
}

// ---- beams: every line carries the beam, as in a pipeline call after rt_set_rec_beam
int rt_debug_ctc_beam_host(const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line, int n_lines,
                           int beam, int nbest, int32_t* counts_out, rt_beam* beams_out, int32_t* tokens_out) {
  hr::BeamArgs a{{z5, W, bias, N, tokens_per_line, n_lines}};
  a.beam = beam; a.nbest = nbest; a.counts_out = counts_out; a.beams_out = beams_out; a.tokens_out = tokens_out;
  return host_entry("rt_debug_ctc_beam_host", a, hr::beam_ref);
}
RT_API int rt_debug_ctc_beam(rt_session* s, const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line,
                             int n_lines, int beam, int nbest, int chunk_rows, int32_t* counts_out, rt_beam* beams_out,
                             int32_t* tokens_out) {
  hr::BeamArgs a{{z5, W, bias, N, tokens_per_line, n_lines}};
  a.beam = beam; a.nbest = nbest; a.counts_out = counts_out; a.beams_out = beams_out; a.tokens_out = tokens_out;
  if (const int rc = device_check(s, "rt_debug_ctc_beam", a, chunk_rows)) return rc;
  return guarded(s, [&] {
    if (beam == 0 || n_lines == 0) return;   // (off, or no line: no launch, no write)
    TailHook h(s, a, {nullptr, nullptr, 0, chunk_rows, beam, nbest}, std::vector<RecLineOpts>((size_t)n_lines), RecStores{});
    rt_session::RecTail::Beam& t = h.t.beam;
    // (what the kernels write starts as the caller's values: a slot they leave alone comes back untouched)
    const size_t nt = (size_t)std::max<long long>(a.rows, 1) * nbest;
    t.count = h.bufs.upload(counts_out, (size_t)n_lines);
    t.recs = h.bufs.upload(reinterpret_cast<const bm::Beam*>(beams_out), (size_t)n_lines * nbest);
    t.tok = h.bufs.alloc<int>(nt);
    DevBufs::put(t.tok, tokens_out, (size_t)a.rows * nbest);
    h.run();
    DevBufs::download(counts_out, t.count, (size_t)n_lines);
    DevBufs::download(reinterpret_cast<bm::Beam*>(beams_out), t.recs, (size_t)n_lines * nbest);
    DevBufs::download(tokens_out, t.tok, (size_t)a.rows * nbest);
  });
}

// ---- beams with language-model fusion (ctc_lm.h): the model in its id form, compiled by the check; its tables go to the device
// as rt_lm_create puts them
int rt_debug_lm_compile(const void* dict, size_t dict_len, const char* arpa, size_t len, float oov_log10, int32_t* ngram_ids_out,
                        int ids_cap, int32_t* ngram_lens_out, float* logp_out, float* backoff_out, int n_cap, int* n_ids_out, int* n_out,
                        int* order_out, int* dropped_out, int* states_out, float* oov_out, int* n_classes, char* err, size_t err_cap) {
  const bool bad = (!dict && dict_len) || (!arpa && len) || !n_ids_out || !n_out || !order_out || !dropped_out || !states_out || !oov_out ||
                   !n_classes || ids_cap < 0 || n_cap < 0 || (!ngram_ids_out && ids_cap) || ((!ngram_lens_out || !logp_out || !backoff_out) && n_cap);
  if (!bad) { *n_ids_out = 0; *n_out = 0; *order_out = 0; *dropped_out = 0; *states_out = 0; *oov_out = 0.0f; }
  return compile_hook("rt_debug_lm_compile", bad, dict, dict_len, n_classes, err, err_cap, [&](const std::vector<std::string>& d) {
    lm::Ids f; lm::Model m; std::string msg;
    const int rc = lm::compile_arpa(d, arpa, len, oov_log10, f, m, msg);
    if (rc != lm::OK) throw RtError(rc, msg);
    *n_ids_out = (int)f.ids.size(); *n_out = f.n(); *order_out = m.order; *dropped_out = m.dropped; *states_out = (int)m.states.size(); *oov_out = m.oov;
    if ((size_t)ids_cap < f.ids.size() || n_cap < f.n())
      throw RtError(RT_ERR_INVALID, "rt_debug_lm_compile: the model needs " + std::to_string(f.ids.size()) + " ids and " + std::to_string(f.n()) + " n-grams");
    memcpy(ngram_ids_out, f.ids.data(), f.ids.size() * sizeof(int32_t));
    memcpy(ngram_lens_out, f.lens.data(), f.lens.size() * sizeof(int32_t));
    memcpy(logp_out, f.logp.data(), f.logp.size() * sizeof(float));
    memcpy(backoff_out, f.backoff.data(), f.backoff.size() * sizeof(float));
  });
}
int rt_debug_lm_score(int classes, const int32_t* ngram_ids, const int32_t* ngram_lens, const float* logp, const float* backoff, int n,
                      float oov, const int32_t* strings, const int32_t* string_lens, int n_strings, float* lm_out, int32_t* state_out,
                      char* err, size_t err_cap) {
  if (err && err_cap) err[0] = 0;
  auto refuse = [&](const std::string& why) {
    if (err && err_cap) snprintf(err, err_cap, "rt_debug_lm_score: %s", why.c_str());
    return RT_ERR_INVALID;
  };
  if (n_strings < 0 || (n_strings > 0 && (!strings || !string_lens || !lm_out || !state_out))) return refuse("bad argument");
  try {
    lm::Model m;
    const std::string bad = hr::IdModel{ngram_ids, ngram_lens, logp, backoff, n, oov}.compile(classes, m);
    if (!bad.empty()) return refuse(bad);
    long long o = 0;
    for (int i = 0; i < n_strings; i++) {
      if (string_lens[i] < 0) return refuse("string " + std::to_string(i) + " has a negative length");
      for (int k = 0; k < string_lens[i]; k++)
        if (strings[o + k] < 1 || strings[o + k] >= classes)
          return refuse("class id " + std::to_string(strings[o + k]) + " in string " + std::to_string(i) + " is outside [1, " + std::to_string(classes) + ")");
      o += string_lens[i];
    }
    const lm::View v = m.view();
    o = 0;
    for (int i = 0; i < n_strings; i++) {
      const lm::Step x = lm::walk(v, strings + o, string_lens[i]);
      lm_out[i] = x.score; state_out[i] = x.next;
      o += string_lens[i];
    }
    return RT_OK;
  } catch (const std::exception& e) {
    if (err && err_cap) snprintf(err, err_cap, "%s", e.what());
    return RT_ERR_BACKEND;
  }
}
int rt_debug_ctc_beam_lm_host(const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line, int n_lines,
                              int beam, int nbest, const int32_t* ngram_ids, const int32_t* ngram_lens, const float* logp,
                              const float* backoff, int n, float oov, float alpha, float beta, int32_t* counts_out, rt_beam* beams_out,
                              int32_t* tokens_out, rt_beam_lm* lm_out) {
  hr::BeamLmArgs a;
  static_cast<hr::Head&>(a) = hr::Head{z5, W, bias, N, tokens_per_line, n_lines};
  a.beam = beam; a.nbest = nbest; a.counts_out = counts_out; a.beams_out = beams_out; a.tokens_out = tokens_out;
  a.ids = {ngram_ids, ngram_lens, logp, backoff, n, oov}; a.alpha = alpha; a.beta = beta; a.lm_out = lm_out;
  return host_entry("rt_debug_ctc_beam_lm_host", a, hr::beam_lm_ref);
}
RT_API int rt_debug_ctc_beam_lm(rt_session* s, const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line,
                                int n_lines, int beam, int nbest, int chunk_rows, const int32_t* ngram_ids, const int32_t* ngram_lens,
                                const float* logp, const float* backoff, int n, float oov, float alpha, float beta, int32_t* counts_out,
                                rt_beam* beams_out, int32_t* tokens_out, rt_beam_lm* lm_out) {
  hr::BeamLmArgs a;
  static_cast<hr::Head&>(a) = hr::Head{z5, W, bias, N, tokens_per_line, n_lines};
  a.beam = beam; a.nbest = nbest; a.counts_out = counts_out; a.beams_out = beams_out; a.tokens_out = tokens_out;
  a.ids = {ngram_ids, ngram_lens, logp, backoff, n, oov}; a.alpha = alpha; a.beta = beta; a.lm_out = lm_out;
  if (const int rc = device_check(s, "rt_debug_ctc_beam_lm", a, chunk_rows)) return rc;
  return guarded(s, [&] {
    if (beam == 0 || n_lines == 0) return;   // (off, or no line: no launch, no write)
    TailHook h(s, a, {nullptr, nullptr, 0, chunk_rows, beam, nbest}, std::vector<RecLineOpts>((size_t)n_lines), RecStores{});
    rt_session::RecTail::Beam& t = h.t.beam;
    // (what the kernels write starts as the caller's values: a slot they leave alone comes back untouched)
    const size_t nt = (size_t)std::max<long long>(a.rows, 1) * nbest;
    t.count = h.bufs.upload(counts_out, (size_t)n_lines);
    t.recs = h.bufs.upload(reinterpret_cast<const bm::Beam*>(beams_out), (size_t)n_lines * nbest);
    t.lms = h.bufs.upload(reinterpret_cast<const lm::BeamLm*>(lm_out), (size_t)n_lines * nbest);
    t.tok = h.bufs.alloc<int>(nt);
    DevBufs::put(t.tok, tokens_out, (size_t)a.rows * nbest);
    const lm::Model& m = a.model;
    t.fused = true;
    t.fu = lm::Fusion{lm::View{h.bufs.upload(m.uni.data(), m.uni.size()), h.bufs.upload(m.states.data(), m.states.size()),
                               h.bufs.upload(m.arcs.data(), m.arcs.size()), m.classes, (int32_t)m.states.size(), (int32_t)m.arcs.size(), m.start},
                      alpha, beta};
    h.run();
    DevBufs::download(counts_out, t.count, (size_t)n_lines);
    DevBufs::download(reinterpret_cast<bm::Beam*>(beams_out), t.recs, (size_t)n_lines * nbest);
    DevBufs::download(reinterpret_cast<lm::BeamLm*>(lm_out), t.lms, (size_t)n_lines * nbest);
    DevBufs::download(tokens_out, t.tok, (size_t)a.rows * nbest);
  });
}

// ---- beams with a word list (ctc_vocab.h): the vocabulary in its id form, compiled by the check; its tables go to the device as
// rt_vocab_create puts them
int rt_debug_vocab_compile(const void* dict, size_t dict_len, const char* utf8, size_t len, int flags, int32_t* word_ids_out, int ids_cap,
                           int32_t* word_lens_out, int n_cap, int* n_ids_out, int* n_out, int* words_out, int* nodes_out,
                           int* word_classes_out, int* variants_dropped_out, int* n_classes, char* err, size_t err_cap) {
  const bool bad = (!dict && dict_len) || (!utf8 && len) || !n_ids_out || !n_out || !words_out || !nodes_out || !word_classes_out ||
                   !variants_dropped_out || !n_classes || ids_cap < 0 || n_cap < 0 || (!word_ids_out && ids_cap) || (!word_lens_out && n_cap);
  if (!bad) { *n_ids_out = 0; *n_out = 0; *words_out = 0; *nodes_out = 0; *word_classes_out = 0; *variants_dropped_out = 0; }
  return compile_hook("rt_debug_vocab_compile", bad, dict, dict_len, n_classes, err, err_cap, [&](const std::vector<std::string>& d) {
    vc::Ids f;
    const vc::Vocab m = rt::compile_vocab(d, utf8, len, nullptr, nullptr, 0, flags, f);
    *n_ids_out = (int)f.ids.size(); *n_out = f.n(); *words_out = m.n_words; *nodes_out = (int)m.nodes.size();
    *word_classes_out = m.n_word_classes; *variants_dropped_out = m.variants_dropped;
    if ((size_t)ids_cap < f.ids.size() || n_cap < f.n())
      throw RtError(RT_ERR_INVALID, "rt_debug_vocab_compile: the vocabulary needs " + std::to_string(f.ids.size()) + " ids and " + std::to_string(f.n()) + " words");
    memcpy(word_ids_out, f.ids.data(), f.ids.size() * sizeof(int32_t));
    memcpy(word_lens_out, f.lens.data(), f.lens.size() * sizeof(int32_t));
  });
}
int rt_debug_vocab_walk(int classes, const int32_t* word_ids, const int32_t* word_lens, int n_words, const int32_t* strings,
                        const int32_t* string_lens, int n_strings, int32_t* open_out, int32_t* closed_out, int32_t* state_out, char* err,
                        size_t err_cap) {
  if (err && err_cap) err[0] = 0;
  auto refuse = [&](int code, const std::string& why) {
    if (err && err_cap) snprintf(err, err_cap, "rt_debug_vocab_walk: %s", why.c_str());
    return code;
  };
  if (n_strings < 0 || (n_strings > 0 && (!strings || !string_lens || !open_out || !closed_out || !state_out))) return refuse(RT_ERR_INVALID, "bad argument");
  if (n_words < 0 || (n_words > 0 && (!word_ids || !word_lens))) return refuse(RT_ERR_INVALID, "the vocabulary's arrays are null or n_words is negative");
  try {
    vc::Vocab m; std::string msg;
    const int rc = vc::compile(classes, word_ids, word_lens, n_words, m, msg);
    if (rc != vc::OK) return refuse(rc, msg);
    long long o = 0;
    for (int i = 0; i < n_strings; i++) {
      if (string_lens[i] < 0) return refuse(RT_ERR_INVALID, "string " + std::to_string(i) + " has a negative length");
      for (int k = 0; k < string_lens[i]; k++)
        if (strings[o + k] < 1 || strings[o + k] >= classes)
          return refuse(RT_ERR_INVALID, "class id " + std::to_string(strings[o + k]) + " in string " + std::to_string(i) + " is outside [1, " + std::to_string(classes) + ")");
      o += string_lens[i];
    }
    const vc::View v = m.view();
    o = 0;
    for (int i = 0; i < n_strings; i++) {
      const vc::Walk x = vc::walk(v, strings + o, string_lens[i]);
      open_out[i] = x.oov; closed_out[i] = x.closed; state_out[i] = x.state;
      o += string_lens[i];
    }
    return RT_OK;
  } catch (const std::exception& e) {
    if (err && err_cap) snprintf(err, err_cap, "%s", e.what());
    return RT_ERR_BACKEND;
  }
}
namespace {
void fill_vocab_args(hr::BeamVocabArgs& a, const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line, int n_lines,
          int beam, int nbest, const int32_t* ngram_ids, const int32_t* ngram_lens, const float* logp, const float* backoff, int n,
          float oov, float alpha, float beta, const int32_t* word_ids, const int32_t* word_lens, int n_words, float gamma,
          int32_t* counts_out, rt_beam* beams_out, int32_t* tokens_out, rt_beam_lm* lm_out, rt_beam_vocab* vocab_out) {
  static_cast<hr::Head&>(a) = hr::Head{z5, W, bias, N, tokens_per_line, n_lines};
  a.beam = beam; a.nbest = nbest; a.counts_out = counts_out; a.beams_out = beams_out; a.tokens_out = tokens_out;
  a.ids = {ngram_ids, ngram_lens, logp, backoff, n, oov}; a.alpha = alpha; a.beta = beta; a.lm_out = lm_out;
  a.words = {word_ids, word_lens, n_words}; a.gamma = gamma; a.vocab_out = vocab_out;
}
}  // namespace
int rt_debug_ctc_beam_vocab_host(const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line, int n_lines,
                                 int beam, int nbest, const int32_t* ngram_ids, const int32_t* ngram_lens, const float* logp,
                                 const float* backoff, int n, float oov, float alpha, float beta, const int32_t* word_ids,
                                 const int32_t* word_lens, int n_words, float gamma, int32_t* counts_out, rt_beam* beams_out,
                                 int32_t* tokens_out, rt_beam_lm* lm_out, rt_beam_vocab* vocab_out) {
  hr::BeamVocabArgs a;
  fill_vocab_args(a, z5, W, bias, N, tokens_per_line, n_lines, beam, nbest, ngram_ids, ngram_lens, logp, backoff, n, oov, alpha, beta, word_ids,
       word_lens, n_words, gamma, counts_out, beams_out, tokens_out, lm_out, vocab_out);
  return host_entry("rt_debug_ctc_beam_vocab_host", a, hr::beam_vocab_ref);
}
RT_API int rt_debug_ctc_beam_vocab(rt_session* s, const float* z5, const float* W, const float* bias, int N, const int32_t* tokens_per_line,
                                   int n_lines, int beam, int nbest, int chunk_rows, const int32_t* ngram_ids, const int32_t* ngram_lens,
                                   const float* logp, const float* backoff, int n, float oov, float alpha, float beta,
                                   const int32_t* word_ids, const int32_t* word_lens, int n_words, float gamma, int32_t* counts_out,
                                   rt_beam* beams_out, int32_t* tokens_out, rt_beam_lm* lm_out, rt_beam_vocab* vocab_out) {
  hr::BeamVocabArgs a;
  fill_vocab_args(a, z5, W, bias, N, tokens_per_line, n_lines, beam, nbest, ngram_ids, ngram_lens, logp, backoff, n, oov, alpha, beta, word_ids,
       word_lens, n_words, gamma, counts_out, beams_out, tokens_out, lm_out, vocab_out);
  if (const int rc = device_check(s, "rt_debug_ctc_beam_vocab", a, chunk_rows)) return rc;
  return guarded(s, [&] {
    if (beam == 0 || n_lines == 0) return;   // (off, or no line: no launch, no write)
    TailHook h(s, a, {nullptr, nullptr, 0, chunk_rows, beam, nbest}, std::vector<RecLineOpts>((size_t)n_lines), RecStores{});
    rt_session::RecTail::Beam& t = h.t.beam;
    // (what the kernels write starts as the caller's values: a slot they leave alone comes back untouched)
    const size_t nt = (size_t)std::max<long long>(a.rows, 1) * nbest, nr = (size_t)n_lines * nbest;
    const bool fused = a.has_model();
    t.count = h.bufs.upload(counts_out, (size_t)n_lines);
    t.recs = h.bufs.upload(reinterpret_cast<const bm::Beam*>(beams_out), nr);
    t.vocs = h.bufs.upload(reinterpret_cast<const vc::BeamVocab*>(vocab_out), nr);
    t.tok = h.bufs.alloc<int>(nt);
    DevBufs::put(t.tok, tokens_out, (size_t)a.rows * nbest);
    if (fused) {
      const lm::Model& m = a.model;
      t.lms = h.bufs.upload(reinterpret_cast<const lm::BeamLm*>(lm_out), nr);
      t.fused = true;
      t.fu = lm::Fusion{lm::View{h.bufs.upload(m.uni.data(), m.uni.size()), h.bufs.upload(m.states.data(), m.states.size()),
                                 h.bufs.upload(m.arcs.data(), m.arcs.size()), m.classes, (int32_t)m.states.size(), (int32_t)m.arcs.size(), m.start},
                        alpha, beta};
    }
    const vc::Vocab& w = a.vocab;
    t.worded = true;
    t.wc = vc::Constraint{vc::View{h.bufs.upload(w.nodes.data(), w.nodes.size()), h.bufs.upload(w.arcs.data(), w.arcs.size()),
                                   h.bufs.upload(w.mask.data(), w.mask.size()), h.bufs.upload(w.root.data(), w.root.size()), w.classes,
                                   (int32_t)w.nodes.size(), (int32_t)w.arcs.size()},
                          gamma};
    h.run();
    DevBufs::download(counts_out, t.count, (size_t)n_lines);
    DevBufs::download(reinterpret_cast<bm::Beam*>(beams_out), t.recs, nr);
    DevBufs::download(reinterpret_cast<vc::BeamVocab*>(vocab_out), t.vocs, nr);
    if (fused) DevBufs::download(reinterpret_cast<lm::BeamLm*>(lm_out), t.lms, nr);
    DevBufs::download(tokens_out, t.tok, (size_t)a.rows * nbest);
  });
}

}  // extern "C"
