// Lexicon snap: a line whose best lexicon entry is likely enough takes that entry as its decode (rt_lexicon_set_snap), written
// once for the device kernel (k_ctc_lexicon_align: prepost_kernels.hip) and the CPU check (rt_debug_ctc_lexicon_align_host).
// ctc_lexicon.h ranks a caller's word list per line and leaves the line's text alone; here the winner is aligned to the line's
// time steps by a CTC Viterbi pass and the aligned path replaces the line's (idx, prob) rows BEFORE k_ctc_decode, the way a
// charset replaces them (ctc_charset.h).  The keep rule, the score, k_word_boxes, k_ctc_kept_rows and the JSON then run
// unchanged over those rows: the corrected string comes with time steps, word boxes, per-token confidences and a line score.
//
// Notation of ctc_lexicon.h: l[t][c] the recomputed fp32 logits, lse[t] = lse_of(...) over the real classes, the winner e has L
// ids and S = 2 L + 1 states, cls_of / skip_of as there.
//   snap      a lexicon carries min_posterior in [0, 1]; 0 (the default) never snaps.  A line of that lexicon snaps iff
//             min_posterior > 0, its match count is >= 1 and matches[0].posterior >= min_posterior: an fp32 comparison on the
//             value k_ctc_lexicon_topk wrote (snaps()); a NaN never snaps.  The aligned entry is match 0, the FORWARD winner, not
//             the entry with the best Viterbi score.
//   viterbi   in the raw-logit domain, fp32, adds and compares only: lse[t] is the same for every state of a step and cannot
//             change the path, and leaving it out keeps expf / logf out of the argmax -- host and device agree bit for bit
//             wherever their logits do.  v_0[s] = l[0][cls(s)] for s < 2, -inf otherwise; for t >= 1
//             v_t[s] = best(v_{t-1}[s], v_{t-1}[s-1], skip_of(s) ? v_{t-1}[s-2] : -inf) + l[t][cls(s)]   (best()),
//             where best looks at stay, s-1, s-2 in that order and a later argument replaces an earlier one only when it is
//             STRICTLY greater: ties go to stay, then to s-1.  The chosen offset (0, 1, 2) is the state's backpointer of step t.
//   end       state S-1, unless v_{T-1}[S-2] is strictly greater (end_of()); S-2 exists since L >= 1.
//   path      s_{T-1} = end, s_{t-1} = s_t - backpointer_t[s_t].
//   rows      for every row t of the snapped line idx[t] = cls(s_t), prob[t] = expf(l[t][idx[t]] - lse[t]): the FULL softmax,
//             the distribution the lexicon itself reads.
// Why the path exists.  Match 0 is feasible (T >= need, ctc_lexicon.h), so at least one legal state sequence starts in state 0
// or 1 and ends in S-1 or S-2; with finite logits its value is finite, hence v_{T-1}[end] is finite.  By induction a finite
// v_t[s], t >= 1, has a finite chosen predecessor (a sum with -inf is -inf, and best() only moves off `stay` to something
// strictly greater, i.e. finite whenever anything is), and a finite v_0[s] means s < 2.  So backtracking from the end state
// walks finite values down to t = 0 and arrives at a state s < 2.  Whatever the values (a NaN logit included), a backpointer
// never leaves [0, S): offset 1 needs s >= 1 and offset 2 needs skip_of(s), i.e. s >= 3, to have beaten `stay`.
// The greedy decode of a Viterbi path is the entry itself -- equal neighbours are separated by their mandatory blank -- so
// k_ctc_decode returns the entry's ids, a token's time step is the first frame of its run and the line score is the mean of
// prob at those frames.
// With a charset on the same line the charset writes first and a snap that fires overwrites its rows; where it does not fire
// the charset's decode stands.  With candidates on, rank 0 of a snapped token is this (id, prob) pair; ranks >= 1 are what they
// are today (the charset's restriction on that line included).
// Untouched: a line whose snap does not fire, a line of a lexicon with min_posterior = 0 and a line with no lexicon have none
// of their rows written and no value changed; the rt_lexicon_match lists are the same for every line, snapped or not.
// Out of scope: snapping on rt_rec and rt_ctc_decode, a per-region threshold, sharing the logits with the charset pass, and
// aligning entries other than match 0.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "ctc_lexicon.h"

namespace rt {
namespace la {

// the backtrack walks a line in tiles of this many time steps (two 64-bit ballots per step in LDS); a line that fits one tile
// never sends its backpointers through memory
constexpr int TILE = 256;

RT_HD bool snaps(float min_posterior, int n_matches, float posterior) {
  return min_posterior > 0.0f && n_matches >= 1 && posterior >= min_posterior;
}
// the best of stay (a0), s-1 (a1), s-2 (a2; callers pass -inf where the skip is not allowed or the state does not exist);
// *off: which one, 0 / 1 / 2
RT_HD float best(float a0, float a1, float a2, int* off) {
  float b = a0; int o = 0;
  if (a1 > b) { b = a1; o = 1; }
  if (a2 > b) { b = a2; o = 2; }
  *off = o;
  return b;
}
RT_HD int end_of(float v_last, float v_before, int S) { return v_before > v_last ? S - 2 : S - 1; }

// Host reference, plain fp32 loops: aligns one entry (ids [L]) to a line's logits [T][ld] and lse [T], T >= need_of(ids, L);
// idx [T], prob [T] <- the path; returns the end state's Viterbi value
inline float align_line(const float* logits, int ld, const float* lse, int T, const int32_t* ids, int L, int32_t* idx,
                        float* prob) {
  const int S = 2 * L + 1;
  float v[2 * lx::MAX_LEN + 1], nx[2 * lx::MAX_LEN + 1];
  std::vector<uint8_t> bp((size_t)T * S, 0);
  for (int s = 0; s < S; s++) v[s] = s < 2 ? logits[lx::cls_of(ids, s)] : -INFINITY;
  for (int t = 1; t < T; t++) {
    for (int s = 0; s < S; s++) {
      int off;
      const float b = best(v[s], s >= 1 ? v[s - 1] : -INFINITY, s >= 2 && lx::skip_of(ids, s) ? v[s - 2] : -INFINITY, &off);
      nx[s] = b + logits[(size_t)t * ld + lx::cls_of(ids, s)];
      bp[(size_t)t * S + s] = (uint8_t)off;
    }
    for (int s = 0; s < S; s++) v[s] = nx[s];
  }
  int s = end_of(v[S - 1], v[S - 2], S);
  const float vit = v[s];
  for (int t = T - 1; t >= 0; t--) {
    const int c = lx::cls_of(ids, s);
    idx[t] = c;
    prob[t] = expf(logits[(size_t)t * ld + c] - lse[t]);
    s -= bp[(size_t)t * S + s];
  }
  return vit;
}

}  // namespace la
}  // namespace rt
