// The host references of the rec CTC tail's options -- candidates, charsets, lexicons (with lexicon snap), patterns, keywords,
// beams -- and what they require of a call: what the rt_debug_ctc_*_host entries run and what both forms of every rt_debug_ctc_*
// entry check (api_ctc.cpp).  Every GPU test of the tail holds the device to these loops, and the CPU tests hold these loops to
// independent Python references.  One argument struct per kind over the common Head: an entry fills it by name, error() / ok()
// checks it and writes rows (and table), the kind's *_ref function computes from it.  A new rec option adds one struct, one
// callback on walk_lines and two thin entries.  Plain C++ as rec_tail_plan.h: no HIP, no RtError, no session; built and run on
// its own under the sanitizers by tests/test_ctc_host_driver_cpu.py.  Compile with -ffp-contract=off: the outputs are compared
// bit for bit.
#pragma once
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/retto_hip.h"
#include "ctc_beam.h"
#include "ctc_candidates.h"
#include "ctc_charset.h"
#include "ctc_keyword.h"
#include "ctc_lexicon.h"
#include "ctc_lexicon_align.h"
#include "ctc_pattern.h"

namespace rt {
namespace hr {

// the width of the CTC head's input, a row of z5: SvtrCore::D's value (nets.h), which this header cannot include
constexpr int HEAD_D = 120;

inline std::string S(long long v) { return std::to_string(v); }

// What every kind takes: the head's input rows z5 [rows][HEAD_D], its FC W [HEAD_D][N] and bias [N] (as cs::row_logits reads
// them), and the lines' time steps.  rows: their sum, written by the kind's check.
struct Head {
  const float* z5 = nullptr; const float* W = nullptr; const float* bias = nullptr;
  int N = 0;
  const int32_t* tokens_per_line = nullptr;
  int n_lines = 0;
  long long rows = 0;
};

// ---- the shared pieces of the checks; each returns the first requirement that fails, in words, or the empty string -----------
// The line loop: no negative line, every line's id of the kind (line_id, null: the kind has none) in [0, bound], fewer than 2^30
// time steps in all -> h.rows.  first_entry (with line_id): *table = the entries of the lists of the lines that name one.
inline std::string lines_error(Head& h, const int32_t* line_id, int bound, const char* noun, const int32_t* first_entry = nullptr,
                               long long* table = nullptr) {
  long long rows = 0, entries = 0;
  for (int i = 0; i < h.n_lines; i++) {
    if (h.tokens_per_line[i] < 0) return "line " + S(i) + " has a negative number of time steps";
    if (line_id && (line_id[i] < 0 || line_id[i] > bound))
      return "line " + S(i) + " names " + noun + " " + S(line_id[i]) + ", outside [0, " + S(bound) + "]";
    rows += h.tokens_per_line[i];
    if (first_entry && line_id[i] > 0) entries += first_entry[line_id[i]] - first_entry[line_id[i] - 1];
  }
  if (rows >= (1ll << 30)) return "the lines have " + S(rows) + " time steps, 2^30 or more";
  h.rows = rows;
  if (table) *table = entries;
  return std::string();
}

// The lists of a lexicon or keyword call: list k (1-based in a line's id) has the entries [first_entry[k - 1], first_entry[k]),
// entry j has entry_lens[j] class ids, which follow each other in entry_ids.
struct EntryLists {
  const int32_t* entry_ids = nullptr; const int32_t* entry_lens = nullptr; const int32_t* first_entry = nullptr;
  int n = 0;
  int entries() const { return first_entry[n]; }
  // where each entry's ids begin in entry_ids (and, last, where they end)
  std::vector<long long> id_offsets() const {
    std::vector<long long> off((size_t)entries() + 1, 0);
    for (int j = 0; j < entries(); j++) off[(size_t)j + 1] = off[(size_t)j] + entry_lens[j];
    return off;
  }
};
// ... and what is required of them: first_entry[0] = 0, 1 .. RT_LEXICON_MAX_ENTRIES entries a list (a keyword list's min_score,
// where given, a number at most 0), 1 .. RT_LEXICON_MAX_LEN ids an entry, every id a class of [1, N).  noun: "lexicon" or "list";
// prefix: of the arrays' names in the entry's signature, "lex" or "kw".
inline std::string lists_error(const EntryLists& e, int N, const char* noun, const char* prefix, const float* min_score = nullptr) {
  if (e.first_entry[0] != 0) return std::string(prefix) + "_first_entry[0] must be 0";
  for (int k = 0; k < e.n; k++) {
    const long long n = (long long)e.first_entry[k + 1] - e.first_entry[k];
    if (n < 1 || n > RT_LEXICON_MAX_ENTRIES) return std::string(noun) + " " + S(k + 1) + " has " + S(n) + " entries, outside [1, RT_LEXICON_MAX_ENTRIES]";
    if (min_score && !(min_score[k] <= 0.0f))
      return std::string(prefix) + "_min_score[" + S(k) + "] = " + std::to_string(min_score[k]) + " is not a number at most 0";
  }
  long long o = 0;
  for (int j = 0; j < e.entries(); j++) {
    if (e.entry_lens[j] < 1 || e.entry_lens[j] > RT_LEXICON_MAX_LEN)
      return "entry " + S(j) + " has " + S(e.entry_lens[j]) + " ids, outside [1, RT_LEXICON_MAX_LEN]";
    for (int i = 0; i < e.entry_lens[j]; i++)
      if (e.entry_ids[o + i] < 1 || e.entry_ids[o + i] >= N)
        return "class id " + S(e.entry_ids[o + i]) + " in entry " + S(j) + " is outside [1, " + S(N) + ")";
    o += e.entry_lens[j];
  }
  return std::string();
}

// the decoded rows a candidate or charset call hands in: every idx a class
inline bool idx_rows_ok(const int32_t* idx, long long rows, int N) {
  for (long long r = 0; r < rows; r++)
    if (idx[r] < 0 || idx[r] >= N) return false;
  return true;
}

// ---- the host line walk ---------------------------------------------------------------------------------------------------------
// For each line that pick(line) selects: logits [T][N] (cs::row_logits of the line's rows) and stat(row's logits, N) per row --
// lx::row_lse or kw::row_max -- handed to fn(line, first row, T, logits, stats).  The row offset advances for every line.  (A line
// without a time step gets one row of zeros.)
template <class Stat, class Pick, class Fn>
void walk_lines(const Head& h, Stat stat, Pick pick, Fn fn) {
  int max_T = 1;
  for (int i = 0; i < h.n_lines; i++) max_T = std::max(max_T, h.tokens_per_line[i]);
  std::vector<float> logits((size_t)max_T * h.N), stats((size_t)max_T);
  long long o = 0;
  for (int i = 0; i < h.n_lines; i++) {
    const int T = h.tokens_per_line[i];
    if (pick(i)) {
      std::fill_n(logits.begin(), (size_t)std::max(T, 1) * h.N, 0.0f); std::fill_n(stats.begin(), (size_t)std::max(T, 1), 0.0f);
      for (int t = 0; t < T; t++) {
        cs::row_logits(h.z5 + (size_t)(o + t) * HEAD_D, HEAD_D, h.W, h.bias, h.N, logits.data() + (size_t)t * h.N);
        stats[(size_t)t] = stat(logits.data() + (size_t)t * h.N, h.N);
      }
      fn(i, o, T, logits.data(), stats.data());
    }
    o += T;
  }
}

// ---- candidates (ctc_candidates.h) ------------------------------------------------------------------------------------------------
struct CandArgs : Head {
  const int32_t* idx = nullptr; const float* prob = nullptr;
  int K = 0;
  rt_candidate* cands_out = nullptr; int32_t* cols_out = nullptr; int32_t* n_tokens_out = nullptr;
  bool ok() {
    if (!idx || !prob || !tokens_per_line || !cands_out || !cols_out || !n_tokens_out) return false;
    if (n_lines <= 0 || K < 1 || K > RT_MAX_CANDIDATES || N <= 0 || (K > 1 && (!z5 || !W))) return false;
    return lines_error(*this, nullptr, 0, "").empty() && idx_rows_ok(idx, rows, N);
  }
};
inline void candidates_ref(const CandArgs& a) {
  std::vector<float> logits((size_t)a.N);
  cc::Cand* out = reinterpret_cast<cc::Cand*>(a.cands_out);
  const int K = a.K;
  long long o = 0;
  for (int i = 0; i < a.n_lines; i++) {
    const int T = a.tokens_per_line[i];
    const int n = cc::line_kept(a.idx + o, a.prob + o, T, K, a.cols_out + o, out + o * K);
    a.n_tokens_out[i] = n;
    for (int j = 0; K > 1 && j < n; j++) {
      cc::Cand* c = out + (o + j) * K;
      cc::row_candidates(a.z5 + (size_t)(o + a.cols_out[o + j]) * HEAD_D, HEAD_D, a.W, a.bias, a.N, c[0].id, K, c, logits.data());
    }
    o += T;
  }
}

// ---- charsets (ctc_charset.h); K = 0: no candidates, cands / cols may then be null ---------------------------------------------
struct CharsetArgs : Head {
  int32_t* idx = nullptr; float* prob = nullptr;   // in, and out where a line is restricted
  const int32_t* line_set = nullptr; const uint32_t* masks = nullptr;
  int n_sets = 0, K = 0;
  int32_t* tokens_out = nullptr; int32_t* n_tokens_out = nullptr; float* scores_out = nullptr;
  rt_candidate* cands_out = nullptr; int32_t* cols_out = nullptr;
  bool ok() {
    if (!z5 || !W || !idx || !prob || !tokens_per_line || !line_set || !tokens_out || !n_tokens_out || !scores_out) return false;
    if (n_lines <= 0 || N <= 0 || K < 0 || K > RT_MAX_CANDIDATES || n_sets < 0 || n_sets > RT_MAX_CHARSETS || (n_sets > 0 && !masks)) return false;
    if (K > 0 && (!cands_out || !cols_out)) return false;
    return lines_error(*this, line_set, n_sets, "charset").empty() && idx_rows_ok(idx, rows, N);
  }
};
inline void charset_ref(const CharsetArgs& a) {
  const int K = a.K, N = a.N, words = cs::mask_words(N);
  std::vector<float> logits((size_t)N);
  cc::Cand* out = reinterpret_cast<cc::Cand*>(a.cands_out);
  int32_t* idx = a.idx; float* prob = a.prob;
  long long o = 0;
  for (int i = 0; i < a.n_lines; i++) {
    const int T = a.tokens_per_line[i];
    const uint32_t* m = a.line_set[i] > 0 ? a.masks + (size_t)(a.line_set[i] - 1) * words : nullptr;
    for (int t = 0; m && t < T; t++) {   // the restricted rows' (idx, prob), before the decode
      cs::row_logits(a.z5 + (size_t)(o + t) * HEAD_D, HEAD_D, a.W, a.bias, N, logits.data());
      cs::row_argmax(logits.data(), N, m, idx + o + t, prob + o + t, nullptr, nullptr);
    }
    int cnt = 0; float acc = 0.0f;   // k_ctc_decode
    for (int t = 0; t < T; t++)
      if (cc::kept(idx[o + t], t > 0 ? idx[o + t - 1] : 0, t == 0)) { a.tokens_out[o + cnt] = idx[o + t]; acc = acc + prob[o + t]; cnt++; }
    a.n_tokens_out[i] = cnt;
    // (no token: NaN.  A line without a time step gets the constant: a compiler may fold its 0 / 0 into this value or leave it to
    // the processor, whose NaN carries the other sign, and the bits must not depend on the build; an all-blank line's 0 / 0 is
    // the processor's)
    a.scores_out[i] = T > 0 ? acc / (float)(unsigned)cnt : NAN;
    if (K > 0) {
      const int n = cc::line_kept(idx + o, prob + o, T, K, a.cols_out + o, out + o * K);
      for (int j = 0; K > 1 && j < n; j++) {
        cc::Cand* c = out + (o + j) * K;
        const float* z = a.z5 + (size_t)(o + a.cols_out[o + j]) * HEAD_D;
        if (m) { cs::row_logits(z, HEAD_D, a.W, a.bias, N, logits.data()); cs::row_candidates(logits.data(), N, m, c[0].id, K, c); }
        else cc::row_candidates(z, HEAD_D, a.W, a.bias, N, c[0].id, K, c, logits.data());
      }
    }
    o += T;
  }
}

// ---- lexicons (ctc_lexicon.h) and lexicon snap (ctc_lexicon_align.h) ------------------------------------------------------------
struct LexiconArgs : Head {
  const int32_t* line_lex = nullptr;
  EntryLists lists;
  float* loglik_out = nullptr;   // optional
  rt_lexicon_match* matches_out = nullptr; int32_t* n_matches_out = nullptr;
  // the snap forms (rt_debug_ctc_lexicon_align*) alone: a threshold per lexicon, the decoded rows in and out, the flags and the
  // Viterbi values
  bool align = false;
  const float* lex_min_post = nullptr;
  int32_t* idx = nullptr; float* prob = nullptr; int32_t* snapped_out = nullptr; float* vit_out = nullptr;
  long long table = 0;   // the floats of the loglik table: one per entry of the lexicon of every line that has one (the check's)
  std::string error() {
    if (!z5 || !W || !tokens_per_line || !line_lex || !lists.entry_ids || !lists.entry_lens || !lists.first_entry || !matches_out || !n_matches_out)
      return "a required pointer is null";
    if (n_lines <= 0) return "n_lines must be positive";
    if (N <= 1) return "N must be at least 2 (the blank and one class)";
    if (lists.n < 1 || lists.n > RT_MAX_LEXICONS) return "n_lex = " + S(lists.n) + " is outside [1, RT_MAX_LEXICONS]";
    std::string bad = lists_error(lists, N, "lexicon", "lex");
    if (bad.empty()) bad = lines_error(*this, line_lex, lists.n, "lexicon", lists.first_entry, &table);
    if (!bad.empty()) return bad;
    if (table >= (1ll << 30)) return "the loglik table has " + S(table) + " floats, 2^30 or more";
    if (!align) return std::string();
    if (!lex_min_post || !idx || !prob || !snapped_out || !vit_out) return "a required pointer is null";
    for (int k = 0; k < lists.n; k++)
      if (!(lex_min_post[k] >= 0.0f && lex_min_post[k] <= 1.0f))
        return "lex_min_post[" + S(k) + "] = " + std::to_string(lex_min_post[k]) + " is outside [0, 1]";
    return std::string();
  }
};
inline void lexicon_ref(const LexiconArgs& a) {
  const std::vector<long long> id_off = a.lists.id_offsets();
  const int32_t *first = a.lists.first_entry, *ids = a.lists.entry_ids, *lens = a.lists.entry_lens;
  std::vector<float> row((size_t)a.lists.entries());   // (one line's logliks: no list has more entries than all together)
  long long out = 0;
  for (int i = 0; i < a.n_lines; i++) a.n_matches_out[i] = 0;
  walk_lines(a, lx::row_lse, [&](int i) { return a.line_lex[i] > 0; }, [&](int i, long long o, int T, const float* logits, const float* lse) {
    const int e0 = first[a.line_lex[i] - 1], n = first[a.line_lex[i]] - e0;
    for (int e = 0; e < n; e++) row[(size_t)e] = lx::entry_loglik(logits, a.N, lse, T, ids + id_off[(size_t)(e0 + e)], lens[e0 + e]);
    lx::Match* m = reinterpret_cast<lx::Match*>(a.matches_out) + (size_t)i * lx::MATCHES;
    a.n_matches_out[i] = lx::line_matches(row.data(), n, m);
    if (a.loglik_out) memcpy(a.loglik_out + out, row.data(), (size_t)n * sizeof(float));
    out += n;
    if (!a.align) return;
    // lexicon snap; m[0] is read only where the line has a match
    const bool fire = la::snaps(a.lex_min_post[a.line_lex[i] - 1], a.n_matches_out[i], a.n_matches_out[i] >= 1 ? m[0].posterior : 0.0f);
    a.snapped_out[i] = fire ? 1 : 0;
    if (fire)
      a.vit_out[i] = la::align_line(logits, a.N, lse, T, ids + id_off[(size_t)(e0 + m[0].entry)], lens[e0 + m[0].entry], a.idx + o, a.prob + o);
  });
}

// ---- patterns (ctc_pattern.h) -----------------------------------------------------------------------------------------------------
struct PatternArgs : Head {
  const int32_t* line_pat = nullptr;
  // the n_pat compiled patterns' flat tables: pattern k's group_of at [k][N], its delta [S[k]][G[k]] and accept [S[k]] behind
  // pattern k - 1's
  const int32_t* pat_S = nullptr; const int32_t* pat_G = nullptr; const int32_t* group_of = nullptr; const int32_t* delta = nullptr;
  const int32_t* accept = nullptr;
  int n_pat = 0;
  int32_t* idx = nullptr; float* prob = nullptr;   // in, and out where a line matches
  int32_t* matched_out = nullptr; float* vit_out = nullptr; float* logprob_out = nullptr; float* free_out = nullptr;
  std::vector<pt::Rule> rules;   // the patterns as pt::Rule::build checks and lays them out (the check's)
  std::string error() {
    if (!z5 || !W || !tokens_per_line || !line_pat || !pat_S || !pat_G || !group_of || !delta || !accept || !idx || !prob ||
        !matched_out || !vit_out || !logprob_out || !free_out)
      return "a required pointer is null";
    if (n_lines <= 0) return "n_lines must be positive";
    if (N <= 1 || N > 65535) return "N must be in [2, 65535]";
    if (n_pat < 1 || n_pat > RT_MAX_PATTERNS) return "n_pat = " + S(n_pat) + " is outside [1, RT_MAX_PATTERNS]";
    rules.assign((size_t)n_pat, pt::Rule());
    size_t od = 0, oa = 0;
    for (int k = 0; k < n_pat; k++) {
      if (pat_S[k] < 1 || pat_S[k] > RT_PATTERN_MAX_STATES) return "pattern " + S(k + 1) + ": S = " + S(pat_S[k]) + " is outside [1, RT_PATTERN_MAX_STATES]";
      if (pat_G[k] < 1 || pat_G[k] > N) return "pattern " + S(k + 1) + ": G = " + S(pat_G[k]) + " is outside [1, N]";
      const std::string bad = rules[(size_t)k].build(N, pat_S[k], pat_G[k], group_of + (size_t)k * N, delta + od, accept + oa);
      if (!bad.empty()) return "pattern " + S(k + 1) + ": " + bad;
      od += (size_t)pat_S[k] * pat_G[k]; oa += (size_t)pat_S[k];
    }
    return lines_error(*this, line_pat, n_pat, "pattern");
  }
};
inline void pattern_ref(const PatternArgs& a) {
  walk_lines(a, lx::row_lse, [&](int i) { return a.line_pat[i] > 0; }, [&](int i, long long o, int T, const float* logits, const float* lse) {
    const pt::LineResult r = pt::viterbi_line(a.rules[(size_t)a.line_pat[i] - 1], logits, a.N, lse, T, a.idx + o, a.prob + o);
    a.matched_out[i] = r.matched; a.vit_out[i] = r.vit; a.logprob_out[i] = r.logprob; a.free_out[i] = r.free_logprob;
  });
}

// ---- keywords (ctc_keyword.h) -----------------------------------------------------------------------------------------------------
struct KeywordArgs : Head {
  const int32_t* line_kw = nullptr;
  EntryLists lists;
  const float* kw_min_score = nullptr;
  float* score_out = nullptr; int32_t* span_out = nullptr;   // optional
  rt_keyword_hit* hits_out = nullptr; int32_t* n_hits_out = nullptr;
  long long table = 0;   // the entries of the score / span tables (the check's)
  std::string error() {
    if (!z5 || !W || !tokens_per_line || !line_kw || !lists.entry_ids || !lists.entry_lens || !lists.first_entry || !kw_min_score || !hits_out || !n_hits_out)
      return "a required pointer is null";
    if (n_lines <= 0) return "n_lines must be positive";
    if (N <= 1) return "N must be at least 2 (the blank and one class)";
    if (lists.n < 1 || lists.n > RT_MAX_KEYWORD_LISTS) return "n_kw = " + S(lists.n) + " is outside [1, RT_MAX_KEYWORD_LISTS]";
    std::string bad = lists_error(lists, N, "list", "kw", kw_min_score);
    if (bad.empty()) bad = lines_error(*this, line_kw, lists.n, "list", lists.first_entry, &table);
    if (!bad.empty()) return bad;
    if (table > lx::MAX_GROUP_TABLE) return "the score table has " + S(table) + " entries, more than a group's table holds";
    return std::string();
  }
};
inline void keywords_ref(const KeywordArgs& a) {
  const std::vector<long long> id_off = a.lists.id_offsets();
  const int32_t *first = a.lists.first_entry, *ids = a.lists.entry_ids, *lens = a.lists.entry_lens;
  std::vector<float> row((size_t)a.lists.entries());   // (one line's scores and spans: no list has more entries than all together)
  std::vector<int32_t> span(2 * row.size());
  long long out = 0;
  for (int i = 0; i < a.n_lines; i++) a.n_hits_out[i] = 0;
  walk_lines(a, kw::row_max, [&](int i) { return a.line_kw[i] > 0; }, [&](int i, long long, int T, const float* logits, const float* rmax) {
    const int e0 = first[a.line_kw[i] - 1], n = first[a.line_kw[i]] - e0;
    std::fill_n(span.begin(), (size_t)2 * n, -1);
    for (int e = 0; e < n; e++)
      row[(size_t)e] = kw::entry_spot(logits, a.N, rmax, T, ids + id_off[(size_t)(e0 + e)], lens[e0 + e], span.data() + 2 * (size_t)e);
    a.n_hits_out[i] = kw::line_hits(row.data(), span.data(), n, a.kw_min_score[a.line_kw[i] - 1],
                                    reinterpret_cast<kw::Hit*>(a.hits_out) + (size_t)i * kw::HITS);
    if (a.score_out) memcpy(a.score_out + out, row.data(), (size_t)n * sizeof(float));
    if (a.span_out) memcpy(a.span_out + 2 * out, span.data(), (size_t)2 * n * sizeof(int32_t));
    out += n;
  });
}

// ---- beams (ctc_beam.h); beam = 0 (off) and n_lines = 0 pass the check: nothing is computed or written then --------------------
struct BeamArgs : Head {
  int beam = 0, nbest = 0;
  int32_t* counts_out = nullptr; rt_beam* beams_out = nullptr; int32_t* tokens_out = nullptr;
  std::string error() {
    if (!z5 || !W || !tokens_per_line || !counts_out || !beams_out || !tokens_out) return "a required pointer is null";
    if (n_lines < 0) return "n_lines is negative";
    if (N <= 1) return "N must be at least 2 (the blank and one class)";
    if (beam < 0 || beam > RT_MAX_BEAM) return "beam = " + S(beam) + " is outside [0, RT_MAX_BEAM]";
    if (beam > 0 && (nbest < 1 || nbest > std::min(beam, RT_MAX_NBEST)))
      return "nbest = " + S(nbest) + " is outside [1, min(beam, RT_MAX_NBEST)]";
    const std::string bad = lines_error(*this, nullptr, 0, "");
    if (!bad.empty()) return bad;
    if (beam > 0 && n_lines + rows * beam > bm::MAX_GROUP_NODES)
      return "the lines need " + S(n_lines + rows * beam) + " trie nodes, more than a group's trie holds";
    return std::string();
  }
};
inline void beam_ref(const BeamArgs& a) {
  if (a.beam == 0) return;
  walk_lines(a, lx::row_lse, [](int) { return true; }, [&](int i, long long o, int T, const float* logits, const float* lse) {
    a.counts_out[i] = bm::line_beams(logits, a.N, lse, T, a.N, a.beam, a.nbest, reinterpret_cast<bm::Beam*>(a.beams_out) + (size_t)i * a.nbest,
                                     a.tokens_out + o * a.nbest);
  });
}

// ---- beams with language-model fusion (ctc_lm.h): the beam's arguments, the model in its id form over the head's N classes
// (<s> = N), oov as a natural log, the weights; the check compiles the model.  lm_out [n_lines][nbest] beside beams_out
struct IdModel {
  const int32_t* ngram_ids = nullptr; const int32_t* ngram_lens = nullptr; const float* logp = nullptr; const float* backoff = nullptr;
  int n = 0; float oov = 0.0f;
  // the first requirement that fails, or the empty string with the model compiled into m
  std::string compile(int classes, lm::Model& m) const {
    if (n < 0 || (n > 0 && (!ngram_ids || !ngram_lens || !logp || !backoff))) return "the model's arrays are null or n is negative";
    std::string msg;
    return lm::compile(classes, ngram_ids, ngram_lens, logp, backoff, n, nullptr, oov, m, msg) == lm::OK ? std::string() : msg;
  }
};
struct BeamLmArgs : BeamArgs {
  IdModel ids; float alpha = 0.0f, beta = 0.0f;
  rt_beam_lm* lm_out = nullptr;
  lm::Model model;
  std::string error() {
    if (!lm_out) return "a required pointer is null";
    const std::string bad = BeamArgs::error();
    if (!bad.empty()) return bad;
    if (const char* why = lm::check_weights(alpha, beta)) return why;
    return ids.compile(N, model);
  }
};
inline void beam_lm_ref(const BeamLmArgs& a) {
  if (a.beam == 0) return;
  const lm::Fusion f{a.model.view(), a.alpha, a.beta};
  walk_lines(a, lx::row_lse, [](int) { return true; }, [&](int i, long long o, int T, const float* logits, const float* lse) {
    a.counts_out[i] = bm::line_beams(logits, a.N, lse, T, a.N, a.beam, a.nbest, reinterpret_cast<bm::Beam*>(a.beams_out) + (size_t)i * a.nbest,
                                     a.tokens_out + o * a.nbest, &f, reinterpret_cast<lm::BeamLm*>(a.lm_out) + (size_t)i * a.nbest);
  });
}

// ---- beams with a word list (ctc_vocab.h), with or without a model: the fused beam's arguments -- n = 0 n-grams with
// alpha = beta = 0 means no model, and lm_out may be null then -- plus the vocabulary in its id form over the head's N classes
// and gamma; the check compiles both.  vocab_out [n_lines][nbest] beside beams_out
struct IdVocab {
  const int32_t* word_ids = nullptr; const int32_t* word_lens = nullptr; int n = 0;
  // the first requirement that fails, or the empty string with the vocabulary compiled into m
  std::string compile(int classes, vc::Vocab& m) const {
    if (n < 0 || (n > 0 && (!word_ids || !word_lens))) return "the vocabulary's arrays are null or n_words is negative";
    std::string msg;
    return vc::compile(classes, word_ids, word_lens, n, m, msg) == vc::OK ? std::string() : msg;
  }
};
struct BeamVocabArgs : BeamArgs {
  IdModel ids; float alpha = 0.0f, beta = 0.0f;
  rt_beam_lm* lm_out = nullptr;
  IdVocab words; float gamma = 0.0f;
  rt_beam_vocab* vocab_out = nullptr;
  lm::Model model; vc::Vocab vocab;
  bool has_model() const { return ids.n != 0 || alpha != 0.0f || beta != 0.0f; }
  std::string error() {
    if (!vocab_out || (has_model() && !lm_out)) return "a required pointer is null";
    const std::string bad = BeamArgs::error();
    if (!bad.empty()) return bad;
    if (const char* why = lm::check_weights(alpha, beta)) return why;
    if (const char* why = vc::check_gamma(gamma)) return why;
    if (has_model()) {
      const std::string m = ids.compile(N, model);
      if (!m.empty()) return m;
    }
    return words.compile(N, vocab);
  }
};
inline void beam_vocab_ref(const BeamVocabArgs& a) {
  if (a.beam == 0) return;
  const lm::Fusion f{a.model.view(), a.alpha, a.beta};
  const vc::Constraint w{a.vocab.view(), a.gamma};
  const bool fused = a.has_model();
  walk_lines(a, lx::row_lse, [](int) { return true; }, [&](int i, long long o, int T, const float* logits, const float* lse) {
    a.counts_out[i] = bm::line_beams(logits, a.N, lse, T, a.N, a.beam, a.nbest, reinterpret_cast<bm::Beam*>(a.beams_out) + (size_t)i * a.nbest,
                                     a.tokens_out + o * a.nbest, fused ? &f : nullptr,
                                     fused ? reinterpret_cast<lm::BeamLm*>(a.lm_out) + (size_t)i * a.nbest : nullptr, &w,
                                     reinterpret_cast<vc::BeamVocab*>(a.vocab_out) + (size_t)i * a.nbest);
  });
}

}  // namespace hr
}  // namespace rt
