// Rec patterns: a line's CTC decode constrained to a regular expression, written once for the device kernel
// (k_ctc_pattern_viterbi: prepost_kernels.hip), the CPU check (rt_debug_ctc_pattern_host) and the text compiler
// (rt_debug_pattern_compile).  For the field whose FORMAT is known -- a date, an amount, a plate -- where a charset admits too
// much, a lexicon of every legal string does not fit and matching the greedy text afterwards can only reject: the result is the
// best CTC path whose collapsed string the pattern accepts, a Viterbi pass over the product of the CTC frame labels and the
// pattern's DFA.  The reference has no counterpart: the rule here is this project's own.  This header needs no HIP header, so a
// stand-alone program can include it (tests/fuzz/fuzz_pattern.cpp).
//
// Pattern language.  UTF-8 text that always matches the WHOLE line.  An atom is a set of class ids of [1, classes):
//   literal   a code point that is no metacharacter: every class whose whole dictionary entry is that one code point (duplicates
//             all join, as in compile_charset; U+0020 is the appended " ").  The metacharacters are \ . [ ] ( ) | ? * + { } ^ -;
//             outside a set `-` is a literal too, and ^ ] { } are syntax errors there
//   [...]     single code points and ranges a-z by code point (both ends must match an entry, a <= z), \d, \c{N} and escaped
//             metacharacters; inside a set only \ ] - ^ are special: ^ directly behind [ complements within [1, classes), and a
//             `-` directly behind [ (or [^) or in front of ] is a literal
//   .         [1, classes)          \d   [0-9]          \c{N}   class id N, the only way to name a multi-code-point entry
//   \ + metacharacter   that literal
// Operators: juxtaposition, |, ( ) for grouping only, and ONE of ? * + {m} {m,} {m,n} (0 <= m <= n <= MAX_REPEAT) behind an
// atom or a group; an empty alternative or group matches the empty string.  No anchors, no back-references, no lazy or stacked
// repeats.  Errors carry the byte offset: ERR_UTF8 for malformed text; ERR_INVALID for a literal or range end that matches no
// entry ("U+XXXX"), an empty set, a syntax error, \c{N} outside [1, classes), a pattern that accepts nothing, more than MAX_BYTES
// of text; ERR_CAPACITY past MAX_STATES or MAX_PAIRS (below) or when the repeats expand to more than MAX_POSITIONS atoms.
//
// Compiled form.  A DFA with start state 0 (position automaton, subset construction in order of discovery, groups ascending).
// States from which no accepting state can be reached are removed, with the arcs into them.  The classes are partitioned into
// G groups: two classes share a group iff they are members of exactly the same atoms; group 0 holds the classes in no atom (and
// the blank) and has no arcs.  Tables: group_of [classes], delta [S][G] (-1: no arc), accept [S].  A PAIR is (q', c) such that
// some state q has delta[q][group_of[c]] == q'; P is the number of distinct pairs.  S <= MAX_STATES and P <= MAX_PAIRS; the
// construction stops as soon as it passes either.  `.{8}` over a 6625-class dictionary exceeds P: a wide set belongs into a
// charset, that is the documented limit.  min_steps is the least T for which the rule below is feasible, computed by the same
// recurrence over all-zero logits, whose values are 0 or -inf: the booleans.
//
// Viterbi.  In the raw-logit domain, fp32, adds and compares only: l[t][c] the recomputed logits (ctc_lexicon.h); lse[t] is the
// same for every state of a step and cannot change the path, so no expf / logf is on the chain.  State values at step t:
//   B_t[q]          the frame is blank and the DFA is in q;
//   C_t[(q', c)]    the frame is class c and the DFA is in q' after consuming c.
// Pairs are ordered by (q', c) ascending, predecessors by q ascending.
//   t = 0     B_0[0] = l[0][0], every other B is -inf; C_0[(q', c)] = l[0][c] where delta[0][group_of[c]] == q', else -inf.
//   top(q)    over the pairs (q, c') whose value is greater than -inf: val1 / cls1 the maximum, ties to the lowest c'; val2 the
//             maximum over the others, ties to the lowest c' again (top_insert()).  Without such a pair val is -inf.
//   into(q,c) B_{t-1}[q], replaced by (cls1(q) != c ? val1(q) : val2(q)) only when that is STRICTLY greater (into_of()).  The
//             != c exclusion is CTC's rule: a class cannot follow itself without a blank.
//   t >= 1    C_t[(q', c)] = l[t][c] + best, best = C_{t-1}[(q', c)] (stay), then into(q, c) for the predecessors q of the pair
//             in ascending order, each replacing only when STRICTLY greater: ties go to stay, then to the lowest q, and within a q
//             to the blank.  B_t[q] = l[t][0] + best, best = B_{t-1}[q], replaced by val1(q) only when strictly greater.
//   end       over the accepting q ascending, B_{T-1}[q] then val1(q) of step T-1; a later candidate replaces an earlier one only
//             when strictly greater.  The line is MATCHED iff the winner is greater than -inf (a NaN never wins a strict comparison).
//   path      follow the backpointers from the end.
//   rows      for every row t of a matched line idx[t] = the path's class, prob[t] = expf(l[t][idx[t]] - lse[t]): the full softmax,
//             as the snap writes it.  Per line also vit = the end value, logprob = vit - sum_t lse[t] and free_logprob =
//             sum_t (max_c l[t][c] - lse[t]), both sums in t order; an unmatched pattern line reports vit = logprob = -inf.
// Backpointers are 16-bit codes: STAY, BLANK | q (from B_{t-1}[q]) or the index of a pair.
// Why the path exists and stays in range.  Call a value LIVE when it is greater than -inf (so no NaN).  x = l + best is live only
// if best is live (-inf + anything is -inf or NaN, NaN + anything NaN).  `best` is the value of the node the backpointer names:
// stay names the node itself; BLANK | q is written with q a predecessor from the pair's own list, q in [0, S); a pair index is
// written only from top(q)'s arguments and only when that value won a strict comparison, hence is live, hence was inserted by
// top_insert with its index in [seg[q], seg[q+1]) inside [0, P).  So whatever the values (a NaN logit included) no code outside
// [0, S) / [0, P) is ever stored, every row t >= 1 of the table is written whole, and from a live end node every step back lands
// on a live node of step t - 1.  At t = 0 the live nodes are B_0[0] and the pairs entered from state 0: the walk ends in a start
// state.  The end node is live because the line is matched, and it is B[q] or top(q)'s first argument for an accepting q.
// The greedy decode of such a path is the string the DFA consumed: an entered class differs from the class before it or follows
// a blank, so k_ctc_decode, the keep rule, the score, k_word_boxes, k_ctc_kept_rows and the JSON run unchanged over the rows, and
// a token's time step is the first frame of its run.
// With a charset on the same line the charset writes first and a match overwrites its rows; an unmatched line (T < min_steps)
// has no row written.  A pattern whose start state accepts may match the all-blank path: the line then has no tokens.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "ctc_lexicon.h"

namespace rt {
namespace pt {

constexpr int MAX_PATTERNS = 16;     // RT_MAX_PATTERNS
constexpr int MAX_STATES = 64;       // RT_PATTERN_MAX_STATES
constexpr int MAX_PAIRS = 4096;      // RT_PATTERN_MAX_PAIRS
constexpr int MAX_BYTES = 1024;      // RT_PATTERN_MAX_BYTES
constexpr int MAX_REPEAT = 64;       // the largest m, n of {m,n}
constexpr int MAX_POSITIONS = 4096;  // atoms of the pattern once its repeats are written out
constexpr int OK = 0, ERR_UTF8 = 5, ERR_INVALID = 8, ERR_CAPACITY = 9;   // RT_OK, RT_ERR_* (include/retto_hip.h)

// backpointer codes (16 bits): a pair index is below BLANK since MAX_PAIRS <= BLANK
constexpr int STAY = 0xFFFF, BLANK = 0x8000, NONE = 0x7fffffff;
// The device kernel keeps a line's backpointers in LDS when T * (P + S) codes fit this many, otherwise in the scratch buffer
// the plan sizes (bp_codes()); either way row t holds P pair codes, then S blank codes, and row 0 is never read as codes
constexpr int BP_LDS = 8192;
RT_HD long long bp_codes(int T, int P, int S) { return (long long)T * (P + S); }

// the best two live values of one state's pairs with their pair indices (NONE: no such pair)
struct Top { float v1, v2; int a1, a2; };
RT_HD Top top_empty() { return Top{-INFINITY, -INFINITY, NONE, NONE}; }
// (v, i) ranks before (w, j): the greater value, then the lower pair index -- within a state that is the lower class
RT_HD bool better(float v, int i, float w, int j) { return v > w || (v == w && i < j); }
// one candidate into the list; callers pass live values only (v > -inf), so the list never holds a NaN
RT_HD void top_insert(Top& t, float v, int i) {
  if (better(v, i, t.v1, t.a1)) { t.v2 = t.v1; t.a2 = t.a1; t.v1 = v; t.a1 = i; }
  else if (better(v, i, t.v2, t.a2)) { t.v2 = v; t.a2 = i; }
}
// into(q, c): b = B_{t-1}[q], cls1 = the class of t.a1 (0 where there is none); *code names the winner
RT_HD float into_of(float b, int q, const Top& t, int cls1, int c, int* code) {
  const bool other = cls1 != c;
  const float cand = other ? t.v1 : t.v2;
  float v = b; int k = BLANK | q;
  if (cand > v) { v = cand; k = other ? t.a1 : t.a2; }
  *code = k;
  return v;
}

// one pattern on the device: its pairs at [pair0, pair0 + P) of the flat pair arrays, seg [S + 1] at seg0 (state q' owns the
// pairs [seg[q'], seg[q' + 1])), its n_pred predecessor bytes at pred0 (a pair's list is [pb, pe) of them); pair indices, seg,
// pb and pe count from the pattern's own first pair / byte
struct Pat { int32_t S, P, pair0, seg0, pred0, n_pred; uint64_t accept; };
struct DevTables { const Pat* pats; const int32_t *pair_c, *pair_pb, *pair_pe, *seg; const uint8_t* preds; };
// one line that carries a pattern: its T rows start at position row0 of the call's compact row list, pat is 0-based, its results
// go to slot (the line's index in the call), its backpointer codes start at bp (in codes) of the chunk's scratch buffer
struct Line { int32_t row0, T, pat, slot; long long bp; };

// The tables one pattern's Viterbi runs on, derived from the compiled form (built by the debug hooks; a session's pattern store
// would hold the same)
struct Rule {
  int classes = 0, S = 0, G = 0, P = 0;
  uint64_t accept = 0;
  std::vector<int32_t> pair_q, pair_c, pair_pb, pair_pe, preds, seg;
  // "" or what is wrong with the tables
  std::string build(int classes_, int S_, int G_, const int32_t* group_of, const int32_t* delta, const int32_t* acc) {
    classes = classes_; S = S_; G = G_; P = 0; accept = 0;
    pair_q.clear(); pair_c.clear(); pair_pb.clear(); pair_pe.clear(); preds.clear(); seg.clear();
    if (classes < 2) return "fewer than 2 classes";
    if (S < 1 || S > MAX_STATES) return "S = " + std::to_string(S) + " is outside [1, RT_PATTERN_MAX_STATES]";
    if (G < 1 || G > classes) return "G = " + std::to_string(G) + " is outside [1, classes]";
    for (int c = 0; c < classes; c++)
      if (group_of[c] < 0 || group_of[c] >= G) return "group_of[" + std::to_string(c) + "] is outside [0, G)";
    if (group_of[0] != 0) return "the blank is not in group 0";
    std::vector<std::vector<int32_t>> from((size_t)S * G);   // [q' * G + g]: the states with an arc of group g into q'
    for (int q = 0; q < S; q++)
      for (int g = 0; g < G; g++) {
        const int to = delta[(size_t)q * G + g];
        if (to < -1 || to >= S) return "delta[" + std::to_string(q) + "][" + std::to_string(g) + "] is outside [-1, S)";
        if (to >= 0 && g == 0) return "group 0 has an arc";
        if (to >= 0) from[(size_t)to * G + g].push_back(q);
      }
    std::vector<int32_t> pb((size_t)S * G, -1);
    for (int q = 0; q < S; q++) {
      if (acc[q]) accept |= 1ull << q;
      seg.push_back(P);
      for (int c = 1; c < classes; c++) {
        const size_t k = (size_t)q * G + group_of[c];
        if (from[k].empty()) continue;
        if (P >= MAX_PAIRS) return "more than RT_PATTERN_MAX_PAIRS (" + std::to_string(MAX_PAIRS) + ") pairs";
        if (pb[k] < 0) { pb[k] = (int32_t)preds.size(); preds.insert(preds.end(), from[k].begin(), from[k].end()); }
        pair_q.push_back(q); pair_c.push_back(c); pair_pb.push_back(pb[k]); pair_pe.push_back(pb[k] + (int32_t)from[k].size());
        P++;
      }
    }
    seg.push_back(P);
    return "";
  }
};

// The device tables of a list of patterns, built on the host
struct Tables {
  std::vector<Pat> pats;
  std::vector<int32_t> pair_c, pair_pb, pair_pe, seg;
  std::vector<uint8_t> preds;
  void add(const Rule& r) {
    pats.push_back(Pat{r.S, r.P, (int32_t)pair_c.size(), (int32_t)seg.size(), (int32_t)preds.size(), (int32_t)r.preds.size(), r.accept});
    pair_c.insert(pair_c.end(), r.pair_c.begin(), r.pair_c.end());
    pair_pb.insert(pair_pb.end(), r.pair_pb.begin(), r.pair_pb.end());
    pair_pe.insert(pair_pe.end(), r.pair_pe.begin(), r.pair_pe.end());
    seg.insert(seg.end(), r.seg.begin(), r.seg.end());
    for (int32_t q : r.preds) preds.push_back((uint8_t)q);
  }
};

// Host reference, plain fp32 loops: the recurrence one step at a time.  A null logits row stands for all-zero logits.
struct Run {
  const Rule& R;
  std::vector<float> B, C, nB, nC;
  std::vector<Top> top; std::vector<int> cls1;
  explicit Run(const Rule& r) : R(r), B((size_t)r.S), C((size_t)r.P), nB((size_t)r.S), nC((size_t)r.P), top((size_t)r.S), cls1((size_t)r.S) {}
  static float at(const float* l, int c) { return l ? l[c] : 0.0f; }
  void tops() {
    for (int q = 0; q < R.S; q++) {
      Top t = top_empty();
      for (int p = R.seg[(size_t)q]; p < R.seg[(size_t)q + 1]; p++) if (C[(size_t)p] > -INFINITY) top_insert(t, C[(size_t)p], p);
      top[(size_t)q] = t; cls1[(size_t)q] = t.a1 == NONE ? 0 : R.pair_c[(size_t)t.a1];
    }
  }
  void init(const float* l) {
    for (int q = 0; q < R.S; q++) B[(size_t)q] = q == 0 ? at(l, 0) : -INFINITY;
    for (int p = 0; p < R.P; p++) C[(size_t)p] = R.preds[(size_t)R.pair_pb[(size_t)p]] == 0 ? at(l, R.pair_c[(size_t)p]) : -INFINITY;
  }
  void step(const float* l, uint16_t* bp /* [P + S], or null */) {
    tops();
    for (int p = 0; p < R.P; p++) {
      const int c = R.pair_c[(size_t)p];
      float best = C[(size_t)p]; int code = STAY;
      for (int j = R.pair_pb[(size_t)p]; j < R.pair_pe[(size_t)p]; j++) {
        const int q = R.preds[(size_t)j];
        int k;
        const float v = into_of(B[(size_t)q], q, top[(size_t)q], cls1[(size_t)q], c, &k);
        if (v > best) { best = v; code = k; }
      }
      nC[(size_t)p] = at(l, c) + best;
      if (bp) bp[p] = (uint16_t)code;
    }
    for (int q = 0; q < R.S; q++) {
      float best = B[(size_t)q]; int code = STAY;
      if (top[(size_t)q].v1 > best) { best = top[(size_t)q].v1; code = top[(size_t)q].a1; }
      nB[(size_t)q] = at(l, 0) + best;
      if (bp) bp[R.P + q] = (uint16_t)code;
    }
    B.swap(nB); C.swap(nC);
  }
  float end(int* code) {   // the end value of the current step; *code its node (NONE: unmatched)
    tops();
    float best = -INFINITY; int k = NONE;
    for (int q = 0; q < R.S; q++) {
      if (!((R.accept >> q) & 1ull)) continue;
      if (B[(size_t)q] > best) { best = B[(size_t)q]; k = BLANK | q; }
      if (top[(size_t)q].v1 > best) { best = top[(size_t)q].v1; k = top[(size_t)q].a1; }
    }
    *code = k;
    return best;
  }
};
inline int min_steps_of(const Rule& R) {   // 0: no T is feasible (a trimmed DFA always has one within 2 S + 1 steps)
  Run r(R);
  r.init(nullptr);
  for (int T = 1; T <= 2 * R.S + 1; T++) {
    int code;
    if (r.end(&code) > -INFINITY) return T;
    r.step(nullptr, nullptr);
  }
  return 0;
}
struct LineResult { int matched; float vit, logprob, free_logprob; };
// Host reference: one pattern line over its logits [T][ld] and lse [T]; a matched line's idx [T] and prob [T] are written
inline LineResult viterbi_line(const Rule& R, const float* logits, int ld, const float* lse, int T, int32_t* idx, float* prob) {
  LineResult out{0, -INFINITY, -INFINITY, 0.0f};
  float sum_lse = 0.0f;
  for (int t = 0; t < T; t++) {
    float mx = -INFINITY;
    for (int c = 0; c < R.classes; c++) if (logits[(size_t)t * ld + c] > mx) mx = logits[(size_t)t * ld + c];
    out.free_logprob = out.free_logprob + (mx - lse[t]);
    sum_lse = sum_lse + lse[t];
  }
  if (T < 1) return out;
  const int W = R.P + R.S;
  std::vector<uint16_t> bp((size_t)T * W, (uint16_t)STAY);
  Run r(R);
  r.init(logits);
  for (int t = 1; t < T; t++) r.step(logits + (size_t)t * ld, bp.data() + (size_t)t * W);
  int node;
  const float vit = r.end(&node);
  if (!(vit > -INFINITY)) return out;
  out.matched = 1; out.vit = vit; out.logprob = vit - sum_lse;
  for (int t = T - 1; t >= 0; t--) {
    const int c = (node & BLANK) ? 0 : R.pair_c[(size_t)node];
    idx[t] = c;
    prob[t] = expf(logits[(size_t)t * ld + c] - lse[t]);
    if (t > 0) {
      const int k = bp[(size_t)t * W + ((node & BLANK) ? R.P + (node & ~BLANK) : node)];
      if (k != STAY) node = k;
    }
  }
  return out;
}

// ---- the text compiler -----------------------------------------------------------------------------------------------------
struct Compiled {
  int classes = 0, S = 0, G = 0, P = 0, min_steps = 0;
  std::vector<int32_t> group_of, delta, accept;   // [classes], [S][G], [S]
};
struct Fail { int code; std::string msg; };

inline int utf8_strict(const unsigned char* p, size_t n, uint32_t* cp) {  // bytes consumed, 0 = invalid (Rust's from_utf8 rule)
  if (n == 0) return 0;
  const unsigned char c = p[0];
  if (c < 0x80) { *cp = c; return 1; }
  auto cont = [&](size_t i) { return i < n && (p[i] & 0xC0) == 0x80; };
  if (c >= 0xC2 && c <= 0xDF) { if (!cont(1)) return 0; *cp = ((c & 0x1Fu) << 6) | (p[1] & 0x3Fu); return 2; }
  if (c >= 0xE0 && c <= 0xEF) {
    if (!cont(1) || !cont(2)) return 0;
    if (c == 0xE0 && p[1] < 0xA0) return 0;
    if (c == 0xED && p[1] >= 0xA0) return 0;
    *cp = ((c & 0x0Fu) << 12) | ((p[1] & 0x3Fu) << 6) | (p[2] & 0x3Fu); return 3;
  }
  if (c >= 0xF0 && c <= 0xF4) {
    if (!cont(1) || !cont(2) || !cont(3)) return 0;
    if (c == 0xF0 && p[1] < 0x90) return 0;
    if (c == 0xF4 && p[1] >= 0x90) return 0;
    *cp = ((c & 0x07u) << 18) | ((p[1] & 0x3Fu) << 12) | ((p[2] & 0x3Fu) << 6) | (p[3] & 0x3Fu); return 4;
  }
  return 0;
}

namespace detail {
typedef std::vector<int32_t> Set;   // sorted class ids
typedef std::vector<uint64_t> Bits;
inline bool bit(const Bits& b, int i) { return (b[(size_t)i >> 6] >> (i & 63)) & 1ull; }
inline void set_bit(Bits& b, int i) { b[(size_t)i >> 6] |= 1ull << (i & 63); }
inline void or_into(Bits& a, const Bits& b) { for (size_t i = 0; i < a.size(); i++) a[i] |= b[i]; }

enum Kind { EPS, ATOM, CAT, ALT, STAR, PLUS, OPT };
struct Node { int kind, a, b, atom; };

struct Parser {
  const std::vector<std::string>& dict;
  const unsigned char* s; size_t n, i = 0;
  int classes;
  std::vector<std::pair<uint32_t, int32_t>> single;   // (code point, class) of the one-code-point entries, sorted
  std::vector<Node> nodes;
  std::vector<Set> atoms;                              // unique class sets
  std::map<Set, int> atom_id;
  int positions = 0, depth = 0;

  Parser(const std::vector<std::string>& d, const char* utf8, size_t len) : dict(d), s((const unsigned char*)utf8), n(len), classes((int)d.size()) {
    for (int c = 1; c < classes; c++) {   // (class 0 is the blank, whatever its placeholder text)
      const std::string& e = dict[(size_t)c];
      uint32_t cp;
      if (!e.empty() && (size_t)utf8_strict((const unsigned char*)e.data(), e.size(), &cp) == e.size()) single.push_back({cp, c});
    }
    std::sort(single.begin(), single.end());
  }
  [[noreturn]] void fail(int code, const std::string& what, size_t at) const {
    throw Fail{code, "pattern: " + what + " (byte offset " + std::to_string(at) + ")"};
  }
  static std::string uplus(uint32_t cp) { char b[24]; snprintf(b, sizeof b, "U+%04X", (unsigned)cp); return b; }
  static bool meta(uint32_t c) {
    return c == '\\' || c == '.' || c == '[' || c == ']' || c == '(' || c == ')' || c == '|' || c == '?' || c == '*' || c == '+' ||
           c == '{' || c == '}' || c == '^' || c == '-';
  }
  uint32_t next_cp() {   // the code point at i, consumed
    uint32_t cp;
    const int k = utf8_strict(s + i, n - i, &cp);
    if (k == 0) fail(ERR_UTF8, "the text is not valid UTF-8", i);
    i += (size_t)k;
    return cp;
  }
  bool peek(char c) const { return i < n && s[i] == (unsigned char)c; }
  int node(int kind, int a = -1, int b = -1, int atom = -1) {
    if (nodes.size() >= (size_t)4 * MAX_POSITIONS)
      fail(ERR_CAPACITY, "the repeats expand to more than " + std::to_string(4 * MAX_POSITIONS) + " nodes", i);
    if (kind == ATOM && ++positions > MAX_POSITIONS)
      fail(ERR_CAPACITY, "the repeats expand to more than " + std::to_string(MAX_POSITIONS) + " atoms", i);
    nodes.push_back(Node{kind, a, b, atom});
    return (int)nodes.size() - 1;
  }
  int atom_node(Set set, size_t at) {
    std::sort(set.begin(), set.end());
    set.erase(std::unique(set.begin(), set.end()), set.end());
    if (set.empty()) fail(ERR_INVALID, "an empty set", at);
    auto it = atom_id.find(set);
    if (it == atom_id.end()) { it = atom_id.emplace(set, (int)atoms.size()).first; atoms.push_back(set); }
    return node(ATOM, -1, -1, it->second);
  }
  void add_cp(Set& out, uint32_t cp, size_t at) const {
    auto lo = std::lower_bound(single.begin(), single.end(), std::make_pair(cp, (int32_t)0));
    if (lo == single.end() || lo->first != cp) fail(ERR_INVALID, uplus(cp) + " matches no dictionary entry", at);
    for (; lo != single.end() && lo->first == cp; ++lo) out.push_back(lo->second);
  }
  void add_range(Set& out, uint32_t a, uint32_t z, size_t at_a, size_t at_z) const {
    Set probe;
    add_cp(probe, a, at_a); add_cp(probe, z, at_z);   // (both ends must exist)
    if (a > z) fail(ERR_INVALID, "syntax error: the range " + uplus(a) + "-" + uplus(z) + " is reversed", at_a);
    for (auto lo = std::lower_bound(single.begin(), single.end(), std::make_pair(a, (int32_t)0)); lo != single.end() && lo->first <= z; ++lo)
      out.push_back(lo->second);
  }
  int number(size_t at) {   // decimal digits at i
    if (i >= n || s[i] < '0' || s[i] > '9') fail(ERR_INVALID, "syntax error: a number is expected", i);
    long v = 0;
    while (i < n && s[i] >= '0' && s[i] <= '9') { v = v * 10 + (s[i] - '0'); if (v > 1000000) fail(ERR_INVALID, "syntax error: the number is too large", at); i++; }
    return (int)v;
  }
  // what stands behind a backslash (i past it): a set's worth of classes
  void escape(Set& out, size_t at) {
    if (i >= n) fail(ERR_INVALID, "syntax error: a backslash ends the pattern", at);
    if (s[i] == 'd') { i++; add_range(out, '0', '9', at, at); return; }
    if (s[i] == 'c') {
      i++;
      if (!peek('{')) fail(ERR_INVALID, "syntax error: \\c needs {N}", at);
      i++;
      const int id = number(at);
      if (!peek('}')) fail(ERR_INVALID, "syntax error: \\c{N is not closed", at);
      i++;
      if (id < 1 || id >= classes) fail(ERR_INVALID, "\\c{" + std::to_string(id) + "} is outside [1, " + std::to_string(classes) + ")", at);
      out.push_back(id);
      return;
    }
    const size_t at_cp = i;
    const uint32_t cp = next_cp();
    if (!meta(cp)) fail(ERR_INVALID, "syntax error: " + uplus(cp) + " cannot be escaped", at);
    add_cp(out, cp, at_cp);
  }
  int set_atom(size_t at) {   // i past '['
    Set in;
    bool neg = false;
    if (peek('^')) { neg = true; i++; }
    bool first = true;
    for (;;) {
      if (i >= n) fail(ERR_INVALID, "syntax error: the set is not closed", at);
      if (s[i] == ']') { i++; break; }
      const size_t at_a = i;
      if (s[i] == '\\') { i++; escape(in, at_a); first = false; continue; }
      const uint32_t a = next_cp();
      if (a == '-' && !(first || peek(']'))) fail(ERR_INVALID, "syntax error: a range without its first end", at_a);
      first = false;
      if (peek('-') && i + 1 < n && s[i + 1] != ']') {   // a range a-z
        i++;
        const size_t at_z = i;
        if (s[i] == '\\') {
          i++;
          if (i >= n) fail(ERR_INVALID, "syntax error: a backslash ends the pattern", at_z);
          const uint32_t z = next_cp();
          if (!meta(z)) fail(ERR_INVALID, "syntax error: a range cannot end in a class escape", at_z);
          add_range(in, a, z, at_a, at_z);
        } else {
          add_range(in, a, next_cp(), at_a, at_z);
        }
        continue;
      }
      add_cp(in, a, at_a);
    }
    if (!neg) return atom_node(in, at);
    std::sort(in.begin(), in.end());
    Set out;
    for (int c = 1; c < classes; c++) if (!std::binary_search(in.begin(), in.end(), c)) out.push_back(c);
    return atom_node(out, at);
  }
  int clone(int r) {
    const Node nd = nodes[(size_t)r];   // (a copy: node() may reallocate)
    if (nd.kind == EPS) return node(EPS);
    if (nd.kind == ATOM) return node(ATOM, -1, -1, nd.atom);
    const int a = clone(nd.a), b = nd.b >= 0 ? clone(nd.b) : -1;
    return node(nd.kind, a, b);
  }
  int cat(int a, int b) { return a < 0 ? b : node(CAT, a, b); }
  int repeat(int r, int m, int x /* -1: no upper end */) {
    int out = -1;
    bool used = false;
    auto copy = [&] { const int c = used ? clone(r) : r; used = true; return c; };
    for (int j = 0; j < m; j++) out = cat(out, copy());
    if (x < 0) out = cat(out, node(STAR, copy()));
    else for (int j = m; j < x; j++) out = cat(out, node(OPT, copy()));
    return out < 0 ? node(EPS) : out;
  }
  int parse_atom() {   // -1: no atom starts here
    if (i >= n) return -1;
    const size_t at = i;
    const unsigned char c = s[i];
    if (c == '|' || c == ')') return -1;
    if (c == '(') {
      i++;
      if (++depth > 200) fail(ERR_INVALID, "syntax error: groups nest deeper than 200", at);
      const int r = parse_alt();
      depth--;
      if (!peek(')')) fail(ERR_INVALID, "syntax error: the group is not closed", at);
      i++;
      return r;
    }
    if (c == '[') { i++; return set_atom(at); }
    if (c == '.') { i++; Set all; for (int k = 1; k < classes; k++) all.push_back(k); return atom_node(all, at); }
    if (c == '\\') { i++; Set set; escape(set, at); return atom_node(set, at); }
    if (c == '?' || c == '*' || c == '+' || c == '{') fail(ERR_INVALID, "syntax error: nothing to repeat", at);
    if (c == ']' || c == '}' || c == '^') fail(ERR_INVALID, std::string("syntax error: an unescaped ") + (char)c, at);
    Set set;
    add_cp(set, next_cp(), at);
    return atom_node(set, at);
  }
  int parse_repeat() {
    int r = parse_atom();
    if (r < 0 || i >= n) return r;
    const size_t at = i;
    const unsigned char c = s[i];
    if (c == '?') { i++; r = node(OPT, r); }
    else if (c == '*') { i++; r = node(STAR, r); }
    else if (c == '+') { i++; r = node(PLUS, r); }
    else if (c == '{') {
      i++;
      const int m = number(at);
      int x = m;
      if (peek(',')) { i++; x = peek('}') ? -1 : number(at); }
      if (!peek('}')) fail(ERR_INVALID, "syntax error: the repeat is not closed", at);
      i++;
      if (m > MAX_REPEAT || x > MAX_REPEAT || (x >= 0 && m > x))
        fail(ERR_INVALID, "syntax error: a repeat needs 0 <= m <= n <= " + std::to_string(MAX_REPEAT), at);
      r = repeat(r, m, x);
    } else return r;
    if (i < n && (s[i] == '?' || s[i] == '*' || s[i] == '+' || s[i] == '{'))
      fail(ERR_INVALID, "syntax error: no lazy or stacked repeats", i);
    return r;
  }
  int parse_concat() {
    int out = -1;
    for (;;) {
      const int r = parse_repeat();
      if (r < 0) break;
      out = cat(out, r);
    }
    return out < 0 ? node(EPS) : out;
  }
  int parse_alt() {
    int out = parse_concat();
    while (peek('|')) { i++; const int r = parse_concat(); out = node(ALT, out, r); }
    return out;
  }
};
}  // namespace detail

// A pattern's compiled form over the dictionary `dict` (class 0 the blank, the last one " "): OK, or the status with `err`
inline int compile(const std::vector<std::string>& dict, const char* utf8, size_t len, Compiled& out, std::string& err) {
  using namespace detail;
  out = Compiled();
  out.classes = (int)dict.size();
  try {
    if (len > (size_t)MAX_BYTES)
      throw Fail{ERR_INVALID, "pattern: " + std::to_string(len) + " bytes of text, more than RT_PATTERN_MAX_BYTES (" + std::to_string(MAX_BYTES) + ") (byte offset " + std::to_string(MAX_BYTES) + ")"};
    if (out.classes < 2) throw Fail{ERR_INVALID, "pattern: the dictionary has no class (byte offset 0)"};
    Parser ps(dict, utf8, len);
    const int root = ps.parse_alt();
    if (ps.i < len) ps.fail(ERR_INVALID, ps.s[ps.i] == ')' ? "syntax error: an unopened )" : "syntax error", ps.i);
    const int classes = out.classes, npos = ps.positions + 1, words = (npos + 63) / 64;   // position 0 is the start
    // groups: classes with the same atom memberships, numbered by their lowest class; group 0 the classes in no atom
    std::vector<std::vector<int>> sig((size_t)classes);
    for (size_t u = 0; u < ps.atoms.size(); u++) for (int c : ps.atoms[u]) sig[(size_t)c].push_back((int)u);
    std::map<std::vector<int>, int> group_id;
    group_id[std::vector<int>()] = 0;
    std::vector<std::vector<int>> group_sig(1);
    std::vector<int> group_size(1, 0);
    out.group_of.assign((size_t)classes, 0);
    for (int c = 1; c < classes; c++) {
      auto it = group_id.find(sig[(size_t)c]);
      if (it == group_id.end()) { it = group_id.emplace(sig[(size_t)c], (int)group_sig.size()).first; group_sig.push_back(sig[(size_t)c]); group_size.push_back(0); }
      out.group_of[(size_t)c] = it->second; group_size[(size_t)it->second]++;
    }
    const int G = (int)group_sig.size();
    // the position automaton: nullable / first / last per node (children come before their parents), follow per position
    const size_t nn = ps.nodes.size();
    std::vector<uint8_t> nullable(nn, 0);
    std::vector<Bits> first(nn, Bits((size_t)words, 0)), last(nn, Bits((size_t)words, 0)), follow((size_t)npos, Bits((size_t)words, 0));
    std::vector<int> pos_atom((size_t)npos, -1);
    auto link = [&](const Bits& from, const Bits& to) { for (int p = 1; p < npos; p++) if (bit(from, p)) or_into(follow[(size_t)p], to); };
    int np = 0;
    std::vector<int> order;   // post-order from the root (a clone's source may sit behind its parent in the vector)
    { std::vector<std::pair<int, int>> st; st.push_back({root, 0});
      while (!st.empty()) {
        auto& top = st.back();
        const Node& nd = ps.nodes[(size_t)top.first];
        if (top.second == 0) { top.second = 1; if (nd.a >= 0) { st.push_back({nd.a, 0}); continue; } }
        if (top.second == 1) { top.second = 2; if (nd.b >= 0) { st.push_back({nd.b, 0}); continue; } }
        order.push_back(top.first); st.pop_back();
      } }
    for (int k : order) {
      const Node& nd = ps.nodes[(size_t)k];
      switch (nd.kind) {
        case EPS: nullable[(size_t)k] = 1; break;
        case ATOM: ++np; pos_atom[(size_t)np] = nd.atom; set_bit(first[(size_t)k], np); set_bit(last[(size_t)k], np); break;
        case CAT:
          link(last[(size_t)nd.a], first[(size_t)nd.b]);
          first[(size_t)k] = first[(size_t)nd.a]; if (nullable[(size_t)nd.a]) or_into(first[(size_t)k], first[(size_t)nd.b]);
          last[(size_t)k] = last[(size_t)nd.b]; if (nullable[(size_t)nd.b]) or_into(last[(size_t)k], last[(size_t)nd.a]);
          nullable[(size_t)k] = nullable[(size_t)nd.a] && nullable[(size_t)nd.b];
          break;
        case ALT:
          first[(size_t)k] = first[(size_t)nd.a]; or_into(first[(size_t)k], first[(size_t)nd.b]);
          last[(size_t)k] = last[(size_t)nd.a]; or_into(last[(size_t)k], last[(size_t)nd.b]);
          nullable[(size_t)k] = nullable[(size_t)nd.a] || nullable[(size_t)nd.b];
          break;
        default:   // STAR, PLUS, OPT
          if (nd.kind != OPT) link(last[(size_t)nd.a], first[(size_t)nd.a]);
          first[(size_t)k] = first[(size_t)nd.a]; last[(size_t)k] = last[(size_t)nd.a];
          nullable[(size_t)k] = nd.kind == PLUS ? nullable[(size_t)nd.a] : 1;
      }
    }
    follow[0] = first[(size_t)root];
    Bits fin = last[(size_t)root];
    if (nullable[(size_t)root]) set_bit(fin, 0);
    // per group the positions whose atom holds it
    std::vector<Bits> pos_of((size_t)G, Bits((size_t)words, 0));
    for (int g = 1; g < G; g++)
      for (int p = 1; p <= np; p++)
        if (std::binary_search(group_sig[(size_t)g].begin(), group_sig[(size_t)g].end(), pos_atom[(size_t)p])) set_bit(pos_of[(size_t)g], p);
    // subset construction; it stops as soon as it passes a limit
    std::vector<Bits> states;
    std::map<Bits, int> state_id;
    Bits start((size_t)words, 0); set_bit(start, 0);
    states.push_back(start); state_id[start] = 0;
    std::vector<int32_t> delta;
    std::vector<uint8_t> entered;   // [q' * G + g]
    int pairs = 0;
    for (size_t q = 0; q < states.size(); q++) {
      Bits f((size_t)words, 0);
      for (int p = 0; p < npos; p++) if (bit(states[q], p)) or_into(f, follow[(size_t)p]);
      delta.resize((q + 1) * G, -1);
      for (int g = 1; g < G; g++) {
        Bits nx = f;
        bool any = false;
        for (int w = 0; w < words; w++) { nx[(size_t)w] &= pos_of[(size_t)g][(size_t)w]; any = any || nx[(size_t)w]; }
        if (!any) continue;
        auto it = state_id.find(nx);
        if (it == state_id.end()) {
          if ((int)states.size() >= MAX_STATES)
            throw Fail{ERR_CAPACITY, "pattern: more than RT_PATTERN_MAX_STATES (" + std::to_string(MAX_STATES) + ") states: reached " +
                                         std::to_string(states.size() + 1) + " (byte offset " + std::to_string(len) + ")"};
          it = state_id.emplace(nx, (int)states.size()).first; states.push_back(nx);
        }
        delta[q * G + g] = it->second;
        const size_t e = (size_t)it->second * G + g;
        if (entered.size() <= e) entered.resize(e + 1, 0);
        if (!entered[e]) {
          entered[e] = 1; pairs += group_size[(size_t)g];
          if (pairs > MAX_PAIRS)
            throw Fail{ERR_CAPACITY, "pattern: more than RT_PATTERN_MAX_PAIRS (" + std::to_string(MAX_PAIRS) + ") (state, class) pairs: reached " +
                                         std::to_string(pairs) + "; use a charset for wide sets (byte offset " + std::to_string(len) + ")"};
        }
      }
    }
    int S = (int)states.size();
    std::vector<uint8_t> acc((size_t)S, 0);
    for (int q = 0; q < S; q++) for (int w = 0; w < words; w++) if (states[(size_t)q][(size_t)w] & fin[(size_t)w]) acc[(size_t)q] = 1;
    // trim: keep the states that reach an accepting one
    std::vector<uint8_t> live = acc;
    for (bool grew = true; grew;) {
      grew = false;
      for (int q = 0; q < S; q++)
        for (int g = 1; g < G && !live[(size_t)q]; g++) { const int to = delta[(size_t)q * G + g]; if (to >= 0 && live[(size_t)to]) { live[(size_t)q] = 1; grew = true; } }
    }
    if (!live[0]) throw Fail{ERR_INVALID, "pattern: it accepts nothing (byte offset 0)"};
    std::vector<int> renum((size_t)S, -1);
    int S2 = 0;
    for (int q = 0; q < S; q++) if (live[(size_t)q]) renum[(size_t)q] = S2++;
    out.delta.assign((size_t)S2 * G, -1); out.accept.assign((size_t)S2, 0);
    for (int q = 0; q < S; q++) {
      if (!live[(size_t)q]) continue;
      out.accept[(size_t)renum[(size_t)q]] = acc[(size_t)q];
      for (int g = 1; g < G; g++) { const int to = delta[(size_t)q * G + g]; if (to >= 0 && live[(size_t)to]) out.delta[(size_t)renum[(size_t)q] * G + g] = renum[(size_t)to]; }
    }
    out.S = S2; out.G = G;
    Rule R;
    const std::string bad = R.build(classes, out.S, out.G, out.group_of.data(), out.delta.data(), out.accept.data());
    if (!bad.empty()) throw Fail{ERR_INVALID, "pattern: " + bad + " (byte offset 0)"};
    out.P = R.P;
    out.min_steps = min_steps_of(R);
    if (out.min_steps < 1) throw Fail{ERR_INVALID, "pattern: it accepts nothing (byte offset 0)"};
    err.clear();
    return OK;
  } catch (const Fail& f) {
    err = f.msg;
    return f.code;
  }
}

}  // namespace pt
}  // namespace rt
