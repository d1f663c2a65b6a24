// Per-token confidence and top-K alternatives of the rec CTC decode (rt_config.rec_return_candidates = K), written once for the
// device kernels (k_ctc_kept_rows, k_ctc_topk: prepost_kernels.hip) and the CPU check (rt_debug_ctc_candidates_host).  The
// reference returns a token list and one mean score per line and leaves the rest as `// TODO: word_results`
// (retto-core/src/processor/rec_processor.rs:155); the rule here is this project's own.
//
// A line's greedy decode keeps time step t when its argmax is not the blank 0 and differs from the argmax of step t - 1
// (kept(); pp::ctc_decode's rule).  For kept token j of the line, at time step col[j], with class tok[j]:
//   rank 0        (tok[j], prob[row]): the fused CTC head's own argmax and probability, copied bit for bit -- the line's rec score
//                 is the mean of exactly these probabilities;
//   ranks 1..K-1  the classes c != tok[j] of [0, classes), blank included, with the largest RECOMPUTED logit
//                 l_c = sum_k z5[row][k] * W[k][c] + b[c] (fp32), ordered by logit descending, then by id ascending (better());
//   probability   p_c = exp(l_c - max) / sum_c' exp(l_c' - max), max and sum over every class, the greedy one included;
//   fill          with fewer than K - 1 other classes the rest of the row is (-1, 0.0f);
//   K = 1         confidences and columns only: no logit is recomputed.
// Near ties: the recomputed logits come from another GEMM launch than the fused head's, so a runner-up's recomputed probability
// may exceed rank 0's by rounding; rank 0 is the decode's choice by construction.  Ranks >= 1 are repeatable run to run and equal
// across the entry points on one batch, but not bit-invariant to the batch's composition: the logits GEMM's plan may depend on
// the number of kept rows in a chunk.
#pragma once
#include <math.h>
#include <stdint.h>

#include "geom_math.h"

namespace rt {
namespace cc {

constexpr int MAX_K = 8;           // RT_MAX_CANDIDATES
constexpr int CAND_CHUNK = 2048;   // kept rows per logits recompute: [2048][round_up(6625, 4)] f32 = 54 MB, whatever the batch
constexpr int EMPTY_ID = 0x7fffffff;   // a list slot that holds no class yet (loses to every class by id)

// one entry; the same layout as rt_candidate (include/retto_hip.h)
struct Cand { int32_t id; float prob; };

// time step t is kept: v = its argmax, prev = the argmax of step t - 1 (ignored when first)
RT_HD bool kept(int v, int prev, bool first) { return v != 0 && (first || v != prev); }
// (la, ia) ranks before (lb, ib)
RT_HD bool better(float la, int ia, float lb, int ib) { return la > lb || (la == lb && ia < ib); }
RT_HD float prob_of(float l, float mx, float sum) { return expf(l - mx) / sum; }

// Sorted insertion into a best-first list of N (logit, id) pairs: the worst entry leaves.  Every index is a compile-time constant
// after unrolling, so on the device the list stays in registers.
template <int N>
RT_HD void list_insert(float (&L)[N], int (&I)[N], float v, int c) {
  if (!better(v, c, L[N - 1], I[N - 1])) return;
  L[N - 1] = v; I[N - 1] = c;
#pragma unroll
  for (int j = N - 1; j >= 1; j--) {
    if (better(L[j], I[j], L[j - 1], I[j - 1])) {
      const float tl = L[j]; L[j] = L[j - 1]; L[j - 1] = tl;
      const int ti = I[j]; I[j] = I[j - 1]; I[j - 1] = ti;
    }
  }
}

// Host reference, plain fp32 loops.  Kept tokens of one line of T steps: cols[j] and rank 0 -> out[j * K]; returns their number.
inline int line_kept(const int* idx, const float* prob, int T, int K, int* cols, Cand* out) {
  int n = 0;
  for (int t = 0; t < T; t++) {
    if (!kept(idx[t], t > 0 ? idx[t - 1] : 0, t == 0)) continue;
    cols[n] = t; out[(size_t)n * K].id = idx[t]; out[(size_t)n * K].prob = prob[t];
    n++;
  }
  return n;
}
// Host reference: ranks 1..K-1 of one token from its feature row z [D], W [D][N] row-major and bias [N] (or null) -> out[1..K).
inline void row_candidates(const float* z, int D, const float* W, const float* bias, int N, int tok, int K, Cand* out,
                           float* logits /* scratch [N] */) {
  float L[MAX_K - 1]; int I[MAX_K - 1];
  for (int j = 0; j < MAX_K - 1; j++) { L[j] = -INFINITY; I[j] = EMPTY_ID; }
  float mx = -INFINITY;
  for (int c = 0; c < N; c++) {
    float acc = 0.0f;
    for (int k = 0; k < D; k++) acc = acc + z[k] * W[(size_t)k * N + c];
    const float l = acc + (bias ? bias[c] : 0.0f);
    logits[c] = l;
    if (l > mx) mx = l;
    if (c != tok) list_insert(L, I, l, c);
  }
  float sum = 0.0f;
  for (int c = 0; c < N; c++) sum = sum + expf(logits[c] - mx);
  for (int r = 1; r < K; r++) {
    const bool has = I[r - 1] != EMPTY_ID;
    out[r].id = has ? I[r - 1] : -1;
    out[r].prob = has ? prob_of(L[r - 1], mx, sum) : 0.0f;
  }
}

}  // namespace cc
}  // namespace rt
