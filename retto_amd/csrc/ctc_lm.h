// Rec language model: a character n-gram fused into the CTC prefix beam search (rt_lm_create, rt_set_rec_beam_lm), written once
// for the device kernel (k_ctc_beam_search<true>: prepost_kernels.hip) and the host loop (bm::line_beams with a Fusion,
// rt_debug_ctc_beam_lm_host).  Re-ranking an N-best list afterwards is not the same thing: a string pruned at step t cannot come
// back, so the model acts inside every step's selection.  The reference has no counterpart: the rule here is this project's own.
//
// The model is a back-off n-gram over the recogniser's class ids, order 1 .. MAX_ORDER, at most MAX_NGRAMS n-grams.
//   id form    n n-grams: ngram_lens[i] in 1 .. MAX_ORDER ids each, one after the other in ngram_ids, with logp[i] and backoff[i]
//              as NATURAL logs in fp32.  An id is a class of [1, classes) or, first in its n-gram only, the pseudo-class `classes`:
//              the line start <s>, never a token of a hypothesis.  Refused (check_ids()): the blank (0) or any other id, a
//              non-finite number, an n-gram twice, an n-gram of k > 1 ids whose first k - 1 are not an n-gram, n > MAX_NGRAMS: all ERR_INVALID.
//              order = the longest n-gram (1 for none).  oov: the log-probability of a class without a unigram, finite, <= 0.
//   ARPA       parse(): "\data\", "ngram k=count", "\k-grams:" sections of "log10 p <ws> token ... [<ws> log10 backoff]" lines,
//              "\end\"; a token is the UTF-8 text of one dictionary entry (the lowest id wins), "<sp>" the entry that is U+0020,
//              "<s>" the line start; an n-gram with "</s>", with "<s>" past its first place or with a token the dictionary lacks
//              is dropped and counted; "<unk>"'s unigram, if there is one, gives oov (other n-grams with it are dropped); log10
//              values become natural logs in fp64, then fp32.  Every refusal names its line.
//   states     the empty context (state 0) and every n-gram of at most order - 1 ids: the k-th such n-gram of the id form is state
//              k + 1.  A state's back-off state is the longest proper suffix of its context that is a state.
//   score      score(state, c) walks from the state's context ctx: (ctx, c) is an n-gram: acc + its logp; ctx is empty: acc + oov;
//              otherwise acc += ctx's back-off, ctx = its back-off state, again.  acc starts at 0 and is summed in fp32 in that
//              order (step()).
//   next       next(state, c) = the longest suffix of ctx + c that is a state, of at most order - 1 ids.  It is a suffix of the
//              n-gram that matched plus nothing: a longer suffix x + c that is a state would make (x, c) an n-gram, x a state on
//              ctx's back-off chain, and the walk would have matched there.  So every arc carries its own next.
//   start      the state of (<s>) where that is one, else state 0.
// Device form (Model, View): a dense unigram table [classes] of {logp or oov, next}; per other state its back-off, its back-off
// state and a slice of (tok, logp, next) arcs sorted by tok, found by binary search (find_arc(): at most ARC_STEPS halvings).
//
// Fusion.  A beam member carries lm, the fp32 sum of score over its tokens in reading order (0 for the empty string), and its
// state.  A stay keeps both; ext_{j,r} takes lm_j + score(state_j, c) and next(state_j, c).  The merge rule is unchanged: lm and
// state are functions of the STRING alone -- the same scores added in the same reading order from the same start state -- so the
// member a merge folds into already holds the very bits the extension would bring, whichever way the string was reached; nothing
// is added again.  alive() still looks at the CTC total; the order of a step's candidates is by key_of() descending, then
// candidate index (cc::better): the fused score fused_of(total, lm, len, alpha, beta) = total + (alpha * lm + beta * len), kept
// above -inf for a live candidate so that it never ties with a dead one.  alpha >= 0, alpha and beta finite.  A hypothesis'
// logprob stays its CTC total; BeamLm carries lm and the fused score.  alpha = beta = 0 ranks by total + 0: the plain beam.
// A word list beside the model is ctc_vocab.h's (rt_set_rec_beam_vocab): its key is this fused score minus gamma per word that
// is no entry.  Out of scope: per-region models or vocabularies, word-level n-grams or neural models, a charset- or
// pattern-restricted beam.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "ctc_candidates.h"

namespace rt {
namespace lm {

constexpr int MAX_ORDER = 5;            // RT_MAX_LM_ORDER
constexpr int MAX_NGRAMS = 1 << 22;     // RT_MAX_LM_NGRAMS
constexpr int MAX_LMS = 4;              // RT_MAX_LMS
constexpr int ARC_STEPS = 23;           // a slice has at most MAX_NGRAMS < 2^23 arcs
constexpr int OK = 0, ERR_INVALID = 8;  // RT_OK, RT_ERR_INVALID (api_ctc.cpp asserts it)

struct Uni { float logp; int32_t next; };
struct Arc { int32_t tok; float logp; int32_t next; };
struct State { float backoff; int32_t bo, arc0, n_arcs; };
// one hypothesis' record beside bm::Beam; the same layout as rt_beam_lm (include/retto_hip.h)
struct BeamLm { float lm, score; };
// what the kernel and the host loop read: uni [classes], states [n_states] (state 0's slice is empty), arcs [n_arcs]
struct View {
  const Uni* uni; const State* states; const Arc* arcs;
  int32_t classes, n_states, n_arcs, start;
};
struct Fusion { View m; float alpha, beta; };
struct Step { float score; int32_t next; };

// the arc of `tok` in arcs[a0 .. a0 + n), sorted by tok, or -1; every index read is inside the slice
RT_HD int find_arc(const Arc* arcs, int a0, int n, int tok) {
  int lo = 0, hi = n;   // (the answer, if any, is in [lo, hi))
  for (int it = 0; it < ARC_STEPS && lo < hi; it++) {
    const int mid = lo + ((hi - lo) >> 1);
    const int t = arcs[a0 + mid].tok;
    if (t == tok) return a0 + mid;
    if (t < tok) lo = mid + 1; else hi = mid;
  }
  return -1;
}
// score(state, c) and next(state, c).  A state outside [0, n_states) reads as the empty context, a slice is cut to the arcs
// there are, and the walk ends after MAX_ORDER levels whatever the tables hold: a compiled model never needs any of the three.
RT_HD Step step(const View& m, int state, int c) {
  if (c < 1 || c >= m.classes) return Step{0.0f, 0};   // (never a token: the beam's classes are in [1, classes))
  int s = state > 0 && state < m.n_states ? state : 0;
  float acc = 0.0f;
  for (int level = 0; level < MAX_ORDER && s > 0; level++) {
    const State x = m.states[s];
    const int a0 = x.arc0 >= 0 && x.arc0 <= m.n_arcs ? x.arc0 : m.n_arcs;
    const int n = x.n_arcs >= 0 && x.n_arcs <= m.n_arcs - a0 ? x.n_arcs : 0;
    const int a = find_arc(m.arcs, a0, n, c);
    if (a >= 0) return Step{acc + m.arcs[a].logp, m.arcs[a].next};
    acc += x.backoff;
    s = x.bo > 0 && x.bo < m.n_states ? x.bo : 0;   // (a shorter context each time: at most order - 1 levels)
  }
  return Step{acc + m.uni[c].logp, m.uni[c].next};
}
RT_HD float fused_of(float total, float lm, int len, float alpha, float beta) { return total + (alpha * lm + beta * (float)len); }
// what a step's selection orders by: -inf for a dead candidate (bm::alive), else the fused score held above -inf (and a NaN,
// which only an overflow of alpha * lm could give, taken as the lowest)
RT_HD float key_of(float total, float lm, int len, float alpha, float beta) {
  if (!(total > -INFINITY)) return -INFINITY;
  const float f = fused_of(total, lm, len, alpha, beta);
  return f > -FLT_MAX ? f : -FLT_MAX;
}
// what rt_set_rec_beam_lm and the debug hooks hold the weights to: the first requirement that fails, or null
inline const char* check_weights(float alpha, float beta) {
  if (!(alpha >= 0.0f) || !std::isfinite(alpha)) return "alpha is not a finite number at least 0";
  if (!std::isfinite(beta)) return "beta is not finite";
  return nullptr;
}
inline const char* check_oov(float oov) { return std::isfinite(oov) && oov <= 0.0f ? nullptr : "oov is not a finite number at most 0"; }

// ---- the id form and its compiler (host) ---------------------------------------------------------------------------------------
struct Ids {
  std::vector<int32_t> ids, lens;
  std::vector<float> logp, backoff;
  std::vector<int32_t> line;   // parse(): the ARPA line of each n-gram (1-based), for the messages; empty otherwise
  int n() const { return (int)lens.size(); }
};
struct Model {
  int classes = 0, order = 1, n_ngrams = 0, dropped = 0, start = 0;
  float oov = 0.0f;
  std::vector<Uni> uni; std::vector<State> states; std::vector<Arc> arcs;
  View view() const { return View{uni.data(), states.data(), arcs.data(), classes, (int32_t)states.size(), (int32_t)arcs.size(), start}; }
};

inline std::string key_of_ids(const int32_t* p, int n) { return std::string((const char*)p, (size_t)n * sizeof(int32_t)); }

// The id form (arrays of n n-grams; line: null or each n-gram's source line) -> m.  Returns OK, or the code with msg.
inline int compile(int classes, const int32_t* ids, const int32_t* lens, const float* logp, const float* backoff, long long n,
                   const int32_t* line, float oov, Model& m, std::string& msg) {
  auto where = [&](long long i) { return line ? "line " + std::to_string(line[i]) : "n-gram " + std::to_string(i); };
  if (classes < 2) { msg = "lm: the model needs at least 2 classes (the blank and one class)"; return ERR_INVALID; }
  if (const char* why = check_oov(oov)) { msg = std::string("lm: ") + why; return ERR_INVALID; }
  if (n < 0 || n > MAX_NGRAMS) {
    msg = "lm: " + std::to_string(n) + " n-grams, outside [0, RT_MAX_LM_NGRAMS (" + std::to_string(MAX_NGRAMS) + ")]";
    return ERR_INVALID;
  }
  std::vector<long long> off((size_t)n + 1, 0);
  int order = 1;
  for (long long i = 0; i < n; i++) {
    if (lens[i] < 1 || lens[i] > MAX_ORDER) {
      msg = "lm: " + where(i) + ": an n-gram of " + std::to_string(lens[i]) + " tokens, outside [1, RT_MAX_LM_ORDER (" + std::to_string(MAX_ORDER) + ")]";
      return ERR_INVALID;
    }
    off[(size_t)i + 1] = off[(size_t)i] + lens[i];
    order = std::max(order, (int)lens[i]);
  }
  std::unordered_map<std::string, int32_t> at;   // n-gram -> its index
  at.reserve((size_t)n * 2);
  for (long long i = 0; i < n; i++) {
    const int32_t* g = ids + off[(size_t)i];
    for (int k = 0; k < lens[i]; k++) {
      if (g[k] == 0) { msg = "lm: " + where(i) + ": the blank (class 0) is not a token"; return ERR_INVALID; }
      if (g[k] < 0 || g[k] > classes || (g[k] == classes && k > 0)) {
        msg = "lm: " + where(i) + ": token id " + std::to_string(g[k]) + (g[k] == classes ? " (<s>) past the first place" : " is outside [1, " + std::to_string(classes) + "]");
        return ERR_INVALID;
      }
    }
    if (!std::isfinite(logp[i]) || !std::isfinite(backoff[i])) { msg = "lm: " + where(i) + ": a number is not finite"; return ERR_INVALID; }
    if (!at.emplace(key_of_ids(g, lens[i]), (int32_t)i).second) { msg = "lm: " + where(i) + ": the n-gram is there twice"; return ERR_INVALID; }
  }
  for (long long i = 0; i < n; i++)
    if (lens[i] > 1 && !at.count(key_of_ids(ids + off[(size_t)i], lens[i] - 1))) {
      msg = "lm: " + where(i) + ": the n-gram's context (its first " + std::to_string(lens[i] - 1) + " tokens) is not an n-gram";
      return ERR_INVALID;
    }
  // states: 0 = the empty context, then the n-grams of at most order - 1 ids in the id form's order
  std::vector<int32_t> state_of((size_t)n, -1);
  std::vector<long long> gram_of(1, -1);
  for (long long i = 0; i < n; i++)
    if (lens[i] <= order - 1) { state_of[(size_t)i] = (int32_t)gram_of.size(); gram_of.push_back(i); }
  // the longest suffix of g[0 .. k) that is a state, of at most order - 1 ids, proper or not
  auto suffix_state = [&](const int32_t* g, int k, bool proper) {
    for (int b = proper ? 1 : 0; b < k; b++) {
      if (k - b > order - 1) continue;
      const auto it = at.find(key_of_ids(g + b, k - b));
      if (it != at.end() && state_of[(size_t)it->second] >= 0) return state_of[(size_t)it->second];
    }
    return (int32_t)0;
  };
  Model r;
  r.classes = classes; r.order = order; r.n_ngrams = (int)n; r.oov = oov;
  r.uni.assign((size_t)classes, Uni{oov, 0});
  r.states.assign(gram_of.size(), State{0.0f, 0, 0, 0});
  // arcs: the n-grams of 2 or more ids, grouped by the state of their context, sorted by their last id
  std::vector<int32_t> cnt(gram_of.size() + 1, 0);
  std::vector<int32_t> ctx_state((size_t)n, 0);
  for (long long i = 0; i < n; i++) {
    const int32_t* g = ids + off[(size_t)i];
    if (lens[i] == 1) {
      if (g[0] < classes) r.uni[(size_t)g[0]] = Uni{logp[i], suffix_state(g, 1, false)};
      continue;
    }
    ctx_state[(size_t)i] = state_of[(size_t)at[key_of_ids(g, lens[i] - 1)]];   // (a context has at most order - 1 ids: a state)
    cnt[(size_t)ctx_state[(size_t)i] + 1]++;
  }
  for (size_t s = 0; s + 1 < cnt.size(); s++) cnt[s + 1] += cnt[s];
  r.arcs.assign((size_t)cnt.back(), Arc{0, 0.0f, 0});
  std::vector<int32_t> fill(cnt.begin(), cnt.end() - 1);
  for (long long i = 0; i < n; i++) {
    if (lens[i] == 1) continue;
    const int32_t* g = ids + off[(size_t)i];
    r.arcs[(size_t)fill[(size_t)ctx_state[(size_t)i]]++] = Arc{g[lens[i] - 1], logp[i], suffix_state(g, lens[i], false)};
  }
  for (size_t s = 1; s < gram_of.size(); s++) {
    const long long i = gram_of[s];
    r.states[s] = State{backoff[i], suffix_state(ids + off[(size_t)i], lens[i], true), cnt[s], cnt[s + 1] - cnt[s]};
    std::sort(r.arcs.begin() + cnt[s], r.arcs.begin() + cnt[s + 1], [](const Arc& a, const Arc& b) { return a.tok < b.tok; });
  }
  const int32_t bos = classes;
  const auto it = at.find(key_of_ids(&bos, 1));
  r.start = it != at.end() && state_of[(size_t)it->second] >= 0 ? state_of[(size_t)it->second] : 0;
  m = std::move(r);
  return OK;
}
inline int compile(int classes, const Ids& f, float oov, Model& m, std::string& msg) {
  return compile(classes, f.ids.data(), f.lens.data(), f.logp.data(), f.backoff.data(), f.n(), f.line.empty() ? nullptr : f.line.data(), oov, m, msg);
}

// ---- ARPA text -> the id form (host) --------------------------------------------------------------------------------------------
// dict: the recogniser's dictionary, class 0 the blank whatever its placeholder text.  *oov: in, the caller's natural-log value;
// out, <unk>'s unigram where the file has one.  *dropped: the n-grams left out.  Returns OK, or the code with msg.
inline int parse(const std::vector<std::string>& dict, const char* text, size_t len, Ids& out, float* oov, int* dropped, std::string& msg) {
  const int classes = (int)dict.size();
  std::unordered_map<std::string, int32_t> tok;
  for (int c = classes - 1; c >= 1; c--)
    if (!dict[(size_t)c].empty()) tok[dict[(size_t)c]] = c;
  {
    const auto sp = tok.find(" ");
    if (sp != tok.end()) tok["<sp>"] = sp->second;
  }
  out = Ids{};
  *dropped = 0;
  int section = -1;   // -1: before \data\, 0: in \data\, k: in \k-grams:, MAX_ORDER + 1: after \end\.
  bool declared[MAX_ORDER + 1] = {};
  int lineno = 0;
  std::vector<std::string> f;
  auto fail = [&](int code, const std::string& why) { msg = "lm: line " + std::to_string(lineno) + ": " + why; return code; };
  auto number = [&](const std::string& s, double* v) {
    if (s.empty()) return false;
    char* end = nullptr;
    *v = strtod(s.c_str(), &end);
    return end == s.c_str() + s.size();
  };
  for (size_t pos = 0; pos < len;) {
    size_t e = pos;
    while (e < len && text[e] != '\n') e++;
    lineno++;
    f.clear();
    for (size_t i = pos; i < e;) {   // the fields: runs of bytes other than space, tab, CR
      while (i < e && (text[i] == ' ' || text[i] == '\t' || text[i] == '\r')) i++;
      size_t j = i;
      while (j < e && text[j] != ' ' && text[j] != '\t' && text[j] != '\r') j++;
      if (j > i) f.emplace_back(text + i, j - i);
      i = j;
    }
    pos = e + 1;
    if (f.empty() || section > MAX_ORDER) continue;
    const std::string& h = f[0];
    if (f.size() == 1 && h == "\\data\\") {
      if (section != -1) return fail(ERR_INVALID, "a second \\data\\");
      section = 0;
      continue;
    }
    if (section == -1) continue;   // (a preamble is allowed before \data\)
    if (f.size() == 1 && h == "\\end\\") { section = MAX_ORDER + 1; continue; }
    if (f.size() == 1 && h.size() >= 9 && h[0] == '\\' && h.compare(h.size() - 7, 7, "-grams:") == 0) {
      double k = 0;
      if (!number(h.substr(1, h.size() - 8), &k) || k != (int)k || k < 1) return fail(ERR_INVALID, "a section header that names no order");
      if (k > MAX_ORDER) return fail(ERR_INVALID, "order " + std::to_string((int)k) + " is above RT_MAX_LM_ORDER (" + std::to_string(MAX_ORDER) + ")");
      if (!declared[(int)k]) return fail(ERR_INVALID, "a section of order " + std::to_string((int)k) + " that \\data\\ does not declare");
      section = (int)k;
      continue;
    }
    if (section == 0) {
      // "ngram k=count" (also "ngram k = count")
      std::string rest;
      for (size_t i = 1; i < f.size(); i++) rest += f[i];
      const size_t eq = rest.find('=');
      double k = 0, c = 0;
      if (h != "ngram" || eq == std::string::npos || !number(rest.substr(0, eq), &k) || !number(rest.substr(eq + 1), &c) || k != (long long)k || c != (long long)c || k < 1 || c < 0)
        return fail(ERR_INVALID, "not an \"ngram k=count\" line");
      if (k > MAX_ORDER) return fail(ERR_INVALID, "order " + std::to_string((long long)k) + " is above RT_MAX_LM_ORDER (" + std::to_string(MAX_ORDER) + ")");
      declared[(int)k] = true;
      continue;
    }
    const int k = section;
    if ((int)f.size() != k + 1 && (int)f.size() != k + 2)
      return fail(ERR_INVALID, "a " + std::to_string(k) + "-gram line needs " + std::to_string(k + 1) + " or " + std::to_string(k + 2) + " fields, not " + std::to_string(f.size()));
    double lp = 0, bo = 0;
    if (!number(f[0], &lp) || ((int)f.size() == k + 2 && !number(f[(size_t)k + 1], &bo))) return fail(ERR_INVALID, "a number does not parse");
    if (!std::isfinite(lp) || !std::isfinite(bo)) return fail(ERR_INVALID, "a number is not finite");
    const float lpf = (float)(lp * 2.302585092994046), bof = (float)(bo * 2.302585092994046);
    if (!std::isfinite(lpf) || !std::isfinite(bof)) return fail(ERR_INVALID, "a number is not finite");
    if (k == 1 && f[1] == "<unk>") {
      if (!(lpf <= 0.0f)) return fail(ERR_INVALID, "<unk>'s log-probability is above 0");
      *oov = lpf;
      continue;
    }
    int32_t g[MAX_ORDER];
    bool keep = true;
    for (int i = 0; i < k && keep; i++) {
      const std::string& w = f[(size_t)i + 1];
      if (w == "<s>") { g[i] = classes; keep = i == 0; continue; }
      const auto it = w == "</s>" || w == "<unk>" ? tok.end() : tok.find(w);
      if (it == tok.end()) keep = false; else g[i] = it->second;
    }
    if (!keep) { (*dropped)++; continue; }
    if (out.n() >= MAX_NGRAMS) return fail(ERR_INVALID, "more than RT_MAX_LM_NGRAMS (" + std::to_string(MAX_NGRAMS) + ") n-grams");
    out.ids.insert(out.ids.end(), g, g + k); out.lens.push_back(k); out.logp.push_back(lpf); out.backoff.push_back(bof); out.line.push_back(lineno);
  }
  if (section == -1) { lineno = std::max(lineno, 1); return fail(ERR_INVALID, "no \\data\\ section"); }
  if (section <= MAX_ORDER) return fail(ERR_INVALID, "the file ends without \\end\\");
  return OK;
}

// ARPA text -> m, with m.dropped; oov_log10: the caller's out-of-vocabulary log10 probability (finite, at most 0)
inline int compile_arpa(const std::vector<std::string>& dict, const char* text, size_t len, float oov_log10, Ids& f, Model& m, std::string& msg) {
  if (!std::isfinite(oov_log10) || oov_log10 > 0.0f) { msg = "lm: oov_log10 is not a finite number at most 0"; return ERR_INVALID; }
  float oov = (float)((double)oov_log10 * 2.302585092994046);
  int dropped = 0;
  int rc = parse(dict, text, len, f, &oov, &dropped, msg);
  if (rc != OK) return rc;
  rc = compile((int)dict.size(), f, oov, m, msg);
  if (rc == OK) m.dropped = dropped;
  return rc;
}

// a string's lm and final state by walking the compiled arrays: what a beam member of that string carries
inline Step walk(const View& m, const int32_t* s, int n) {
  float lm = 0.0f; int state = m.start;
  for (int i = 0; i < n; i++) { const Step x = step(m, state, s[i]); lm += x.score; state = x.next; }
  return Step{lm, state};
}

}  // namespace lm
}  // namespace rt
