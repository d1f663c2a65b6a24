// Rec beams: the N most probable STRINGS of a line by CTC prefix beam search (rt_set_rec_beam, rt_results_rec_beams), written once
// for the device kernels (k_ctc_beam_topc, k_ctc_beam_search: prepost_kernels.hip) and the CPU check (rt_debug_ctc_beam_host).
// Every other option of the tail answers a closed question or follows one alignment: the greedy decode is the best PATH, the
// candidates exist at the steps it kept, a lexicon ranks a given list, patterns and keywords are Viterbi searches.  A spell
// corrector, a language model or a field validator asks the open one: which strings are likely, each summed over its alignments,
// and how far apart are they.  The reference has no counterpart: the rule here is this project's own.  Like the keywords it only
// READS a line: it goes with every other option and every other result is what it is without it, bit for bit.
//
// For a line of T >= 1 time steps, a beam width B in 1 .. MAX_BEAM and N in 1 .. min(B, MAX_NBEST):
//   l[t][c]    the RECOMPUTED fp32 logit sum_k z5[row][k] * W[k][c] + b[c], exactly what the lexicons compute;
//   lse[t]     log-sum-exp over every class c < classes (lx::row_lse; k_ctc_row_lse); the GEMM's pad columns take no part;
//   lp[t][c]   l[t][c] - lse[t]: the FULL softmax.  The line's charset, if it has one, is NOT applied: the beam reads the model's
//              own distribution;
//   K_t        the up to TOP_C non-blank classes of step t with the largest logits, ordered by cc::better (logit descending, then
//              id ascending); fewer where the head has fewer than TOP_C + 1 classes (row_topc());
//   hypothesis (string, pb, pnb): the fp32 log-probabilities of the string's alignments so far that end in the blank and in a
//              non-blank; its total is lae(pb, pnb, -inf) (total_of());
//   start      the empty string with pb = 0, pnb = -inf;
//   stay       step t, beam members in beam order j = 0 .. n - 1: stay_j keeps the string, pb' = total_j + lp[t][0] (stay_pb()),
//              pnb' = pnb_j + lp[t][last_j] with last_j the string's last class, whether it is in K_t or not; -inf for the empty
//              string (stay_pnb());
//   extend     for the r-th class c of K_t: ext_{j,r} is string_j + c with pb' = -inf and pnb' = (c == last_j ? pb_j : total_j) +
//              lp[t][c] (ext_pnb()): a repeated class needs a blank between the two;
//   merge      where string_j + c IS the string of another beam member j' there is no such candidate: stay_{j'}.pnb' becomes
//              lae(stay_{j'}.pnb', that value, -inf) (merged()), folded in the order (j ascending, then r ascending) -- at most one
//              (j, r) reaches a given j', since strings in a beam are distinct and so are the classes of K_t;
//   selection  candidates whose total is -inf (or a NaN) are dropped (alive()); the new beam is the best B of the rest by total
//              descending, then candidate index ascending (cc::better), the index of stay_j being j and that of ext_{j,r}
//              MAX_BEAM + j * TOP_C + r (ext_index());
//   result     after the last step the first N hypotheses of the beam in its own order, each (tokens, logprob = total), fewer where
//              the beam is smaller.  The empty string is a legitimate hypothesis with 0 tokens.  T = 0: no hypothesis.
// Identity is by string and exact: one string is never twice in a beam.  A hypothesis' logprob sums a subset of its string's
// alignments -- those that stayed inside the beam -- so it never exceeds the string's full CTC forward log-likelihood; with a beam
// that never overflows it IS that likelihood.  Language-model fusion (rt_set_rec_beam_lm) is ctc_lm.h's: with a lm::Fusion
// every member also carries the model's sum over its string and its model state, and "selection" orders by lm::key_of() -- the
// fused score -- in place of the total; everything else above, logprob included, stays.  A word list (rt_set_rec_beam_vocab) is
// ctc_vocab.h's: with a vc::Constraint every member also carries its trie state and its count of words that are no entries,
// "selection" orders by vc::key_of() -- the fused score (or the total) minus gamma per such word -- and "result" ranks the final
// beam once more by the closing key before it takes the first N.  Out of scope: a charset- or pattern-restricted beam,
// per-region widths, models or vocabularies, word-level n-grams, time steps or word boxes of the alternatives.
//
// Device form.  Strings live in a per-line trie of (parent, token) nodes with find-or-create, so that one string always has one
// node: "member j' is string_j + c" is then parent(j') == node_j && last_j' == c.  Only the at most B survivors of a step need
// nodes, so a line has at most nodes_of(T, B) = 1 + T B of them; a node's children hang on a singly linked list (child, next).
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "ctc_lexicon.h"
#include "ctc_lm.h"
#include "ctc_vocab.h"

namespace rt {
namespace bm {

constexpr int MAX_BEAM = 32;    // RT_MAX_BEAM
constexpr int MAX_NBEST = 8;    // RT_MAX_NBEST
constexpr int TOP_C = 8;
constexpr int CANDS = MAX_BEAM + MAX_BEAM * TOP_C;   // the candidate indices of one step
// The trie nodes of one rec group live in the scratch arena until the group's tail has run; a group that would need more fails
// with RT_ERR_CAPACITY (1 GB of nodes: 2 M time steps at B = 32).
constexpr long long MAX_GROUP_NODES = 1ll << 26;

// one hypothesis' record; the same layout as rt_beam (include/retto_hip.h)
struct Beam { float logprob; int32_t n_tokens; };
// one line: lx::Line with lex = the first of its nodes_of(T, B) trie nodes, out = the first of its N * T token slots (hypothesis k's
// tokens at out + k * T), slot = the line's index in the call: its records at [slot * N ...], its count at [slot]
using Line = lx::Line;
// K_t of one row: ids and logits, best first; past the row's count (cc::EMPTY_ID, -inf)
struct TopC { int32_t id[TOP_C]; float logit[TOP_C]; };
// one trie node: its string is its parent's plus tok; child / next: its first child and its next sibling (-1: none).  Node 0 of a
// line is the empty string
struct Node { int32_t parent, tok, child, next; };

RT_HD long long nodes_of(int T, int B) { return 1 + (long long)T * B; }
RT_HD int ext_index(int j, int r) { return MAX_BEAM + j * TOP_C + r; }
RT_HD float total_of(float pb, float pnb) { return lx::lae(pb, pnb, -INFINITY); }
RT_HD float stay_pb(float total, float lp_blank) { return total + lp_blank; }
// last = 0: the empty string (the blank is never a token)
RT_HD float stay_pnb(float pnb, int last, float lp_last) { return last > 0 ? pnb + lp_last : -INFINITY; }
RT_HD float ext_pnb(float pb, float total, bool repeat, float lp_c) { return (repeat ? pb : total) + lp_c; }
RT_HD float merged(float pnb, float v) { return lx::lae(pnb, v, -INFINITY); }
RT_HD bool alive(float total) { return total > -INFINITY; }   // (a NaN is dropped)

// what rt_set_rec_beam and the debug hooks hold (beam, nbest) to, beam = 0 (off) aside: the first requirement that fails, or null
inline const char* check_params(int beam, int nbest) {
  if (beam < 1 || beam > MAX_BEAM) return "beam is outside [1, RT_MAX_BEAM (32)]";
  if (nbest < 1 || nbest > std::min(beam, MAX_NBEST)) return "nbest is outside [1, min(beam, RT_MAX_NBEST (8))]";
  return nullptr;
}

// Host reference, plain fp32 loops: K_t of one row of logits [N]
inline void row_topc(const float* logits, int N, TopC* out) {
  float L[TOP_C]; int I[TOP_C];
  for (int j = 0; j < TOP_C; j++) { L[j] = -INFINITY; I[j] = cc::EMPTY_ID; }
  for (int c = 1; c < N; c++) cc::list_insert(L, I, logits[c], c);
  for (int j = 0; j < TOP_C; j++) { out->id[j] = I[j]; out->logit[j] = I[j] == cc::EMPTY_ID ? -INFINITY : L[j]; }
}
// Host reference: the hypotheses of one line from its logits [T][ld] (N classes) and lse [T] -> out[0 .. count) and hypothesis k's
// tokens at tokens[k * T ...]; returns the count.  Strings are plain vectors here: identity is comparison.  f (with lm_out
// [nbest]): language-model fusion (ctc_lm.h); null: a candidate's key is its total.  w (with vocab_out [nbest]): the word-list
// constraint (ctc_vocab.h) on top of either
inline int line_beams(const float* logits, int ld, const float* lse, int T, int N, int B, int nbest, Beam* out, int32_t* tokens,
                      const lm::Fusion* f = nullptr, lm::BeamLm* lm_out = nullptr, const vc::Constraint* w = nullptr,
                      vc::BeamVocab* vocab_out = nullptr) {
  if (T <= 0) return 0;
  struct Hyp { std::vector<int32_t> s; float pb, pnb, lm; int state, vstate, oov; };
  struct Cand { float total, pb, pnb; int index, j, c; float key, lm; int state, vstate, oov; };
  // a candidate's key from its total, lm, length and count: vc::key_of over the fused score or the total with a word list,
  // lm::key_of with a model alone, the total otherwise
  auto key_of = [&](float total, float lmv, int len, int oov) {
    if (w) return vc::key_of(total, f ? lm::fused_of(total, lmv, len, f->alpha, f->beta) : total, oov, w->gamma);
    return f ? lm::key_of(total, lmv, len, f->alpha, f->beta) : total;
  };
  std::vector<Hyp> beam(1, Hyp{{}, 0.0f, -INFINITY, 0.0f, f ? f->m.start : 0, 0, 0}), next;
  std::vector<Cand> cands;
  for (int t = 0; t < T; t++) {
    const float* l = logits + (size_t)t * ld;
    TopC K;
    row_topc(l, N, &K);
    const int n = (int)beam.size();
    float tot[MAX_BEAM], spb[MAX_BEAM], spnb[MAX_BEAM];
    for (int j = 0; j < n; j++) {
      const Hyp& h = beam[(size_t)j];
      const int last = h.s.empty() ? 0 : h.s.back();
      tot[j] = total_of(h.pb, h.pnb);
      spb[j] = stay_pb(tot[j], l[0] - lse[t]);
      spnb[j] = stay_pnb(h.pnb, last, l[last] - lse[t]);
    }
    cands.clear();
    for (int j = 0; j < n; j++) {
      const Hyp& h = beam[(size_t)j];
      const int last = h.s.empty() ? 0 : h.s.back();
      for (int r = 0; r < TOP_C && K.id[r] != cc::EMPTY_ID; r++) {
        const int c = K.id[r];
        const float v = ext_pnb(h.pb, tot[j], c == last, K.logit[r] - lse[t]);
        int target = -1;
        for (int q = 0; q < n && target < 0; q++) {
          const std::vector<int32_t>& s = beam[(size_t)q].s;
          if (s.size() == h.s.size() + 1 && s.back() == c && std::equal(h.s.begin(), h.s.end(), s.begin())) target = q;
        }
        if (target >= 0) spnb[target] = merged(spnb[target], v);
        else {
          Cand a{total_of(-INFINITY, v), -INFINITY, v, ext_index(j, r), j, c, 0.0f, 0.0f, 0, 0, 0};
          if (f) {
            const lm::Step x = lm::step(f->m, h.state, c);
            a.lm = h.lm + x.score; a.state = x.next;
          }
          if (w) {
            const vc::Step x = vc::step(w->v, h.vstate, c);
            a.vstate = x.next; a.oov = h.oov + x.add;
          }
          a.key = key_of(a.total, a.lm, (int)h.s.size() + 1, a.oov);
          cands.push_back(a);
        }
      }
    }
    for (int j = 0; j < n; j++) {
      const Hyp& h = beam[(size_t)j];
      Cand a{total_of(spb[j], spnb[j]), spb[j], spnb[j], j, j, 0, 0.0f, h.lm, h.state, h.vstate, h.oov};
      a.key = key_of(a.total, a.lm, (int)h.s.size(), a.oov);
      cands.push_back(a);
    }
    cands.erase(std::remove_if(cands.begin(), cands.end(), [](const Cand& a) { return !alive(a.total); }), cands.end());
    std::sort(cands.begin(), cands.end(), [](const Cand& a, const Cand& b) { return cc::better(a.key, a.index, b.key, b.index); });
    next.clear();
    for (size_t i = 0; i < cands.size() && (int)i < B; i++) {
      const Cand& a = cands[i];
      Hyp h{beam[(size_t)a.j].s, a.pb, a.pnb, a.lm, a.state, a.vstate, a.oov};
      if (a.index >= MAX_BEAM) h.s.push_back(a.c);
      next.push_back(std::move(h));
    }
    beam.swap(next);
  }
  // (with a word list: the final beam ranked by the closing key, then beam order)
  const int n = (int)beam.size();
  int order[MAX_BEAM], closed[MAX_BEAM]; float ckey[MAX_BEAM];
  for (int j = 0; j < n; j++) {
    const Hyp& h = beam[(size_t)j];
    order[j] = j;
    closed[j] = w ? h.oov + vc::close(w->v, h.vstate) : 0;
    ckey[j] = w ? key_of(total_of(h.pb, h.pnb), h.lm, (int)h.s.size(), closed[j]) : 0.0f;
  }
  if (w) std::sort(order, order + n, [&](int a, int b) { return cc::better(ckey[a], a, ckey[b], b); });
  const int count = std::min(nbest, n);
  for (int k = 0; k < count; k++) {
    const Hyp& h = beam[(size_t)order[k]];
    out[k] = Beam{total_of(h.pb, h.pnb), (int32_t)h.s.size()};
    const float fused = f ? lm::fused_of(out[k].logprob, h.lm, out[k].n_tokens, f->alpha, f->beta) : out[k].logprob;
    if (f && lm_out) lm_out[k] = lm::BeamLm{h.lm, fused};
    if (w && vocab_out) vocab_out[k] = vc::BeamVocab{closed[order[k]], vc::score_of(fused, closed[order[k]], w->gamma)};
    for (size_t i = 0; i < h.s.size(); i++) tokens[(size_t)k * T + i] = h.s[i];
  }
  return count;
}

}  // namespace bm
}  // namespace rt
