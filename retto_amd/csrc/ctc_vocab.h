// Rec vocabulary: a soft word-list constraint fused into the CTC prefix beam search (rt_vocab_create, rt_set_rec_beam_vocab),
// written once for the device kernel (k_ctc_beam_search<LM, true>: prepost_kernels.hip) and the host loop (bm::line_beams with a
// Constraint, rt_debug_ctc_beam_vocab_host).  It says "this is running text, and its words should be words of this list": a
// language's word list, a product catalogue, a field vocabulary.  An order-5 character model (ctc_lm.h) cannot tell `recieve`
// from `receive`, a whole-line lexicon does not apply to a line of several words, and re-ranking the N-best list afterwards is
// the weaker rule -- a string pruned at step t cannot come back -- so the list acts inside every step's selection, like the
// language model, and composes with it.  The reference has no counterpart: the rule here is this project's own.
//
//   vocabulary  a set of words, each 1 .. MAX_LEN class ids of [1, classes), at most MAX_WORDS of them; a word given twice is one
//               word.  id form: n words, word i of lens[i] ids, one after the other in ids.
//   classes     the WORD classes are exactly the classes that occur in some word; every other non-blank class is a SEPARATOR
//               (digits, punctuation, the space -- whatever the list does not spell with).
//   trie        node 0 is the root; nodes are numbered in order of first creation while the words are inserted in id-form order,
//               id by id; a node is TERMINAL when a word ends there.
//   state       of a string: a node, or OFF (-1): inside a word that has left the trie.  The start state is 0.
//   step        step(state, c) -> (next, add):
//                 c a separator                              -> (0, close(state))
//                 c a word class, state OFF                  -> (OFF, 0)
//                 c a word class, state has a child on c     -> (that child, 0)
//                 c a word class, no such child (root too)   -> (OFF, 1)
//   close       close(state) = 1 if state > 0 and the node is not terminal -- a word ends there that is no entry -- else 0.  The
//               line end closes an open word.
//   oov         a member's int sum of `add` over its tokens in reading order; its closed count is oov + close(state).  A word
//               still open and still on the trie is, optimistically, not counted.
// State and oov are functions of the STRING alone, so the beam's merge rule stays as it is: the member a merge folds into already
// holds the very values (ctc_lm.h "Fusion").
//
// Selection.  With fused = lm::fused_of(total, lm, len, alpha, beta) where a model is attached and the CTC total otherwise, a
// step's candidates are ordered by key_of(): fused - gamma * (float)oov, held above -inf for a live candidate (-inf for a dead
// one: bm::alive still looks at the CTC total), then candidate index (cc::better).  A stay keeps (state, oov); ext_{j,r} takes
// step(state_j, c).  K_t, merge and the trie of strings are the beam's.
// Result.  After the last step the final beam (up to B members) is ranked once more by the CLOSING key -- key_of() with
// oov + close(state) -- then beam order; the first N are the result.  Beam::logprob stays the CTC total, BeamLm what it is
// (its score holds no gamma); BeamVocab carries the closed count and fused - gamma * (float)(closed count).
// gamma is finite and >= 0.  gamma = 0 makes every key the value it was (x - 0.0f) and the closing rank the identity: the
// vocabulary-free beam's bytes.  A line is never left without hypotheses: the constraint only ever subtracts a finite amount.
//
// Device form (Vocab, View): per node {arc0, n_arcs, terminal}; arcs (tok, next) sorted by tok and found by a bounded binary
// search (find_arc(): at most ARC_STEPS halvings); a word-class bitmask of mask_words(classes) words; a dense [classes] child
// table for the root, where the fan-out is largest and most members sit after a space.  Every read is clamped: a state outside
// [0, n_nodes) reads as OFF, a slice is cut to the arcs there are, a child outside (0, n_nodes) reads as none.
// Out of scope: per-region vocabularies, word-level n-grams, a hard (gamma = inf) constraint, case folding beyond CASE_VARIANTS.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "ctc_candidates.h"

namespace rt {
namespace vc {

constexpr int MAX_LEN = 63;             // RT_VOCAB_MAX_LEN
constexpr int MAX_WORDS = 1 << 20;      // RT_VOCAB_MAX_WORDS
constexpr int MAX_VOCABS = 4;           // RT_MAX_VOCABS
constexpr int CASE_VARIANTS = 1;        // RT_VOCAB_CASE_VARIANTS
constexpr int ARC_STEPS = 31;           // a slice has fewer than 2^31 arcs
constexpr int OFF = -1;
constexpr int OK = 0, ERR_INVALID = 8, ERR_CAPACITY = 9;  // RT_OK, RT_ERR_* (api_ctc.cpp asserts it)

struct Node { int32_t arc0, n_arcs, terminal; };
struct Arc { int32_t tok, next; };
// one hypothesis' record beside bm::Beam; the same layout as rt_beam_vocab (include/retto_hip.h)
struct BeamVocab { int32_t oov_words; float score; };
// what the kernel and the host loop read: nodes [n_nodes], arcs [n_arcs], mask [mask_words(classes)], root [classes] (the
// root's child on c, or -1)
struct View {
  const Node* nodes; const Arc* arcs; const uint32_t* mask; const int32_t* root;
  int32_t classes, n_nodes, n_arcs;
};
struct Constraint { View v; float gamma; };
struct Step { int32_t next, add; };

RT_HD int mask_words(int classes) { return (classes + 31) >> 5; }
RT_HD bool is_word_class(const View& v, int c) { return (v.mask[c >> 5] >> (c & 31)) & 1u; }
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
// 1 where a word ends in `state` that is no entry.  (OFF, the root and a state outside the table: 0 -- OFF was counted when the
// word left the trie)
RT_HD int close(const View& v, int state) { return state > 0 && state < v.n_nodes && !v.nodes[state].terminal ? 1 : 0; }
// a child id as the tables give it, or OFF where it is none of (0, n_nodes)
RT_HD int child_of(const View& v, int next) { return next > 0 && next < v.n_nodes ? next : OFF; }
// the table above.  c outside [1, classes) is never a token (the beam's classes are in [1, classes)): the state stays.
RT_HD Step step(const View& v, int state, int c) {
  if (c < 1 || c >= v.classes) return Step{state, 0};
  if (!is_word_class(v, c)) return Step{0, close(v, state)};
  if (state < 0 || state >= v.n_nodes) return Step{OFF, 0};
  int next = OFF;
  if (state == 0) next = child_of(v, v.root[c]);
  else {
    const Node x = v.nodes[state];
    const int a0 = x.arc0 >= 0 && x.arc0 <= v.n_arcs ? x.arc0 : v.n_arcs;
    const int n = x.n_arcs >= 0 && x.n_arcs <= v.n_arcs - a0 ? x.n_arcs : 0;
    const int a = find_arc(v.arcs, a0, n, c);
    if (a >= 0) next = child_of(v, v.arcs[a].next);
  }
  return Step{next, next == OFF ? 1 : 0};
}
// fused: lm::fused_of() with a model, the CTC total without
RT_HD float score_of(float fused, int oov, float gamma) { return fused - gamma * (float)oov; }
// what a step's selection (oov) and the closing rank (oov + close) order by: -inf for a dead candidate (bm::alive on the CTC
// total), else the score held above -inf (a NaN, which only an overflow could give, taken as the lowest): as lm::key_of
RT_HD float key_of(float total, float fused, int oov, float gamma) {
  if (!(total > -INFINITY)) return -INFINITY;
  const float f = score_of(fused, oov, gamma);
  return f > -FLT_MAX ? f : -FLT_MAX;
}
// what rt_set_rec_beam_vocab and the debug hooks hold gamma to: the requirement that fails, or null
inline const char* check_gamma(float gamma) {
  return gamma >= 0.0f && std::isfinite(gamma) ? nullptr : "gamma is not a finite number at least 0";
}

// ---- the id form and its compiler (host) ---------------------------------------------------------------------------------------
struct Ids {
  std::vector<int32_t> ids, lens;
  int n() const { return (int)lens.size(); }
};
struct Vocab {
  int classes = 0, n_words = 0, n_word_classes = 0, variants_dropped = 0;
  std::vector<Node> nodes; std::vector<Arc> arcs; std::vector<uint32_t> mask; std::vector<int32_t> root;
  View view() const { return View{nodes.data(), arcs.data(), mask.data(), root.data(), classes, (int32_t)nodes.size(), (int32_t)arcs.size()}; }
};

// The id form (n words; a word given twice counts once) -> m.  Returns OK, or the code with msg, which names the word.
inline int compile(int classes, const int32_t* ids, const int32_t* lens, long long n, Vocab& m, std::string& msg) {
  if (classes < 2) { msg = "vocab: the vocabulary needs at least 2 classes (the blank and one class)"; return ERR_INVALID; }
  if (n < 1) { msg = "vocab: no word at all"; return ERR_INVALID; }
  long long o = 0;
  for (long long i = 0; i < n; i++) {
    if (lens[i] < 1) { msg = "vocab: word " + std::to_string(i) + " is empty"; return ERR_INVALID; }
    if (lens[i] > MAX_LEN) {
      msg = "vocab: word " + std::to_string(i) + " has " + std::to_string(lens[i]) + " ids, more than RT_VOCAB_MAX_LEN (" + std::to_string(MAX_LEN) + ")";
      return ERR_INVALID;
    }
    for (int k = 0; k < lens[i]; k++) {
      const int32_t c = ids[o + k];
      if (c == 0) { msg = "vocab: word " + std::to_string(i) + ": the blank (class 0) is not a token"; return ERR_INVALID; }
      if (c < 0 || c >= classes) {
        msg = "vocab: word " + std::to_string(i) + ": class id " + std::to_string(c) + " is outside [1, " + std::to_string(classes) + ")";
        return ERR_INVALID;
      }
    }
    o += lens[i];
  }
  Vocab r;
  r.classes = classes;
  r.mask.assign((size_t)mask_words(classes), 0u);
  r.root.assign((size_t)classes, -1);
  // the trie: (parent, tok) -> child, in order of first creation
  std::unordered_map<uint64_t, int32_t> at;
  std::vector<int32_t> par(1, -1), tok(1, 0), term(1, 0);
  o = 0;
  for (long long i = 0; i < n; i++) {
    int32_t s = 0;
    for (int k = 0; k < lens[i]; k++) {
      const int32_t c = ids[o + k];
      r.mask[(size_t)c >> 5] |= 1u << (c & 31);
      const uint64_t key = ((uint64_t)(uint32_t)s << 32) | (uint32_t)c;
      const auto it = at.find(key);
      if (it != at.end()) { s = it->second; continue; }
      const int32_t id = (int32_t)par.size();
      at.emplace(key, id);
      par.push_back(s); tok.push_back(c); term.push_back(0);
      s = id;
    }
    o += lens[i];
    if (!term[(size_t)s]) {
      if (r.n_words >= MAX_WORDS) { msg = "vocab: more than RT_VOCAB_MAX_WORDS (" + std::to_string(MAX_WORDS) + ") words"; return ERR_CAPACITY; }
      term[(size_t)s] = 1; r.n_words++;
    }
  }
  for (int c = 1; c < classes; c++) r.n_word_classes += (r.mask[(size_t)c >> 5] >> (c & 31)) & 1u;
  // arcs grouped by parent (a counting sort over the nodes, which keeps creation order), each slice then sorted by tok
  const size_t nn = par.size();
  std::vector<int32_t> cnt(nn + 1, 0);
  for (size_t q = 1; q < nn; q++) cnt[(size_t)par[q] + 1]++;
  for (size_t s = 0; s < nn; s++) cnt[s + 1] += cnt[s];
  r.arcs.assign(nn - 1, Arc{0, 0});
  std::vector<int32_t> fill(cnt.begin(), cnt.end() - 1);
  for (size_t q = 1; q < nn; q++) r.arcs[(size_t)fill[(size_t)par[q]]++] = Arc{tok[q], (int32_t)q};
  r.nodes.resize(nn);
  for (size_t s = 0; s < nn; s++) {
    r.nodes[s] = Node{cnt[s], cnt[s + 1] - cnt[s], term[s]};
    std::sort(r.arcs.begin() + cnt[s], r.arcs.begin() + cnt[s + 1], [](const Arc& a, const Arc& b) { return a.tok < b.tok; });
  }
  for (int32_t a = 0; a < r.nodes[0].n_arcs; a++) r.root[(size_t)r.arcs[(size_t)a].tok] = r.arcs[(size_t)a].next;
  m = std::move(r);
  return OK;
}
inline int compile(int classes, const Ids& f, Vocab& m, std::string& msg) { return compile(classes, f.ids.data(), f.lens.data(), f.n(), m, msg); }

// a string's open count, closed count and final state by walking the compiled tables: what a beam member of that string carries
struct Walk { int32_t oov, closed, state; };
inline Walk walk(const View& v, const int32_t* s, int n) {
  int oov = 0, state = 0;
  for (int i = 0; i < n; i++) { const Step x = step(v, state, s[i]); oov += x.add; state = x.next; }
  return Walk{oov, oov + close(v, state), state};
}

}  // namespace vc
}  // namespace rt
