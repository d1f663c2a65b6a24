// Rec charsets: a line's CTC decode restricted to the classes its caller allows (rt_charset_create, rt_set_rec_charset,
// rt_run_regions_charsets), written once for the device kernels (k_ctc_charset_argmax, k_ctc_topk<true>: prepost_kernels.hip) and
// the CPU check (rt_debug_ctc_charset_host).  The reference has no counterpart (like word boxes and candidates): the rule here is
// this project's own.
//
// A charset is a set S of class ids that always holds the blank 0 (allowed() forces it, whatever the mask word says), kept as
// ceil(classes / 32) 32-bit words: class c is bit (c & 31) of word (c >> 5).  For every time step (row) of a line that carries S:
//   l_c    the RECOMPUTED fp32 logit sum_k z5[row][k] * W[k][c] + b[c], exactly what the candidates path computes
//          (ctc_candidates.h);
//   idx    the class of S with the largest l_c, ties to the lower id (cc::better);
//   prob   exp(l_idx - mx) / sum_{c in S} exp(l_c - mx), mx = max_{c in S} l_c;
//   classes outside S and the GEMM's pad columns [classes, round_up(classes, 4)) take no part, neither in mx nor in the sum.
// These (idx, prob) replace the fused head's values of the row BEFORE pp::ctc_decode: the keep rule, the score (mean of the kept
// probabilities), word boxes and JSON then run unchanged over them.  With rec_return_candidates = K on such a line rank 0 is the
// decode's (idx, prob) bit for bit, as ever; ranks >= 1 are the best classes of S other than the token, ordered by better(), with
// probabilities over S; (-1, 0.0f) fills the row when S has fewer than K members.  A class outside S is never named: the masked
// kernel skips disallowed columns instead of lowering their logits (list_insert ranks a -inf entry ahead of EMPTY_ID).
// Lines of charset 0 (none) take no part: no row of theirs is gathered, no value of theirs is written.
//
// Batch invariance.  The logits come from nn::gemm with K = 120 and N = the model's class count (nets.cpp: head.fc's width).  What
// follows holds for the 6625 classes of the PP-OCRv4 dictionary (Npad16 = 6640).  gemm_plan.cpp sends that shape to the narrow
// kernel for every M: 6640 is no multiple of 240 (no wide or persistent tile), N is not 128 (no LDS-resident weights), and the
// streaming kernel takes Npad16 <= 64 only.  M changes the grid and, while there are fewer workgroups than twice the CUs, how many
// 16-column tiles a workgroup takes (nt); a column's sum over K runs in the same order whatever nt is, and rows never mix.  So
// under the production plan a restricted line's (idx, prob), and with them its tokens and score, do not depend on what else is in
// the batch or on the chunking.  A class count whose Npad16 is a multiple of 240 (240, 18480) meets production_variant()'s wide
// tiles from 16384 rows on, so there the kernel can change with M; that a row gets the same bits from those routes at K = 120 is
// not measured (test_gemm_routes_are_bit_identical runs K = 240, 128 and 64).  Either way this is a property of today's plan, not
// a promise of the interface: as for candidates ranks >= 1, what is promised is that results are repeatable run to run and equal
// across the entry points on one batch.
#pragma once
#include <math.h>
#include <stdint.h>

#include "ctc_candidates.h"

namespace rt {
namespace cs {

constexpr int MAX_SETS = 64;   // RT_MAX_CHARSETS

RT_HD int mask_words(int classes) { return (classes + 31) / 32; }
// class c belongs to the set of mask m (the blank always does)
RT_HD bool allowed(const uint32_t* m, int c) { return c == 0 || ((m[c >> 5] >> (c & 31)) & 1u) != 0; }
// the membership bits of the four classes 4 v .. 4 v + 3 (bit u = class 4 v + u): they always lie in one word
RT_HD uint32_t allowed4(const uint32_t* m, int v) { return ((m[v >> 3] >> ((4 * v) & 31)) & 15u) | (v == 0 ? 1u : 0u); }

// Host reference, plain fp32 loops: the logits of one feature row z [D] against W [D][N] row-major and bias [N] (or null).
inline void row_logits(const float* z, int D, const float* W, const float* bias, int N, float* logits) {
  for (int c = 0; c < N; c++) {
    float acc = 0.0f;
    for (int k = 0; k < D; k++) acc = acc + z[k] * W[(size_t)k * N + c];
    logits[c] = acc + (bias ? bias[c] : 0.0f);
  }
}
// Host reference: (idx, prob) of one row over the set of mask m; *mx_out / *sum_out: the maximum and the sum over the set
inline void row_argmax(const float* logits, int N, const uint32_t* m, int* idx, float* prob, float* mx_out, float* sum_out) {
  float mx = -INFINITY; int bi = cc::EMPTY_ID;
  for (int c = 0; c < N; c++)
    if (allowed(m, c) && cc::better(logits[c], c, mx, bi)) { mx = logits[c]; bi = c; }
  float sum = 0.0f;
  for (int c = 0; c < N; c++)
    if (allowed(m, c)) sum = sum + expf(logits[c] - mx);
  if (bi == cc::EMPTY_ID) bi = 0;   // (every allowed logit NaN: the blank)
  *idx = bi; *prob = cc::prob_of(mx, mx, sum);
  if (mx_out) *mx_out = mx;
  if (sum_out) *sum_out = sum;
}
// Host reference: ranks 1..K-1 of one token of a restricted row -> out[1..K)
inline void row_candidates(const float* logits, int N, const uint32_t* m, int tok, int K, cc::Cand* out) {
  float L[cc::MAX_K - 1]; int I[cc::MAX_K - 1];
  for (int j = 0; j < cc::MAX_K - 1; j++) { L[j] = -INFINITY; I[j] = cc::EMPTY_ID; }
  float mx = -INFINITY;
  for (int c = 0; c < N; c++) {
    if (!allowed(m, c)) continue;
    if (logits[c] > mx) mx = logits[c];
    if (c != tok) cc::list_insert(L, I, logits[c], c);
  }
  float sum = 0.0f;
  for (int c = 0; c < N; c++)
    if (allowed(m, c)) sum = sum + expf(logits[c] - mx);
  for (int r = 1; r < K; r++) {
    const bool has = I[r - 1] != cc::EMPTY_ID;
    out[r].id = has ? I[r - 1] : -1;
    out[r].prob = has ? cc::prob_of(L[r - 1], mx, sum) : 0.0f;
  }
}

}  // namespace cs
}  // namespace rt
