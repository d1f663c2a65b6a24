// Rec keywords: a caller's keyword list spotted INSIDE every line (rt_keywords_create, rt_set_rec_keywords,
// rt_run_regions_keywords), written once for the device kernels (k_ctc_keyword_spot, k_ctc_keyword_topk: prepost_kernels.hip)
// and the CPU check (rt_debug_ctc_keywords_host).  For the page-level question "where does it say Total, Invoice No, this
// customer's name": a lexicon ranks whole lines only, a pattern .*Total.* over the whole dictionary runs into pt::MAX_PAIRS by
// design, and searching the greedy text afterwards throws the model's probabilities away -- one weak frame, T0tal, loses the hit.
// The reference has no counterpart: the rule here is this project's own.  It is the first option that only READS a line: it
// conflicts with no other option and every other result of the line -- tokens, score, text, word boxes, candidates, lexicon
// matches and snaps, pattern results, JSON -- is what it is without the list, bit for bit.
//
// A keyword list is an ordered list of entries; entry e is a sequence of L_e class ids, 1 <= L_e <= lx::MAX_LEN, never the blank
// 0; equal neighbours are allowed.  It is compiled by the lexicon's compiler (rt::compile_lexicon) and stored as lx::Tables: the
// 16 / 32 / 64-lane buckets by length fit, since an entry needs 2 L - 1 <= 2 L + 1 lanes.  A list carries one min_score <= 0,
// fixed at creation; -INFINITY: report the best hits whatever they score.  For a line of T time steps and an entry k[0..L):
//   l[t][c]   the RECOMPUTED fp32 logit sum_j z5[row][j] * W[j][c] + b[c], exactly what the lexicons compute;
//   rmax[t]   the largest l[t][c] over c < classes (row_max(); k_ctc_row_max); the GEMM's pad columns take no part;
//   d[t][c]   l[t][c] - rmax[t], one fp32 subtraction, <= 0.  A frame outside the keyword takes its argmax class at cost 0;
//   score     the log-ratio of two probabilities: the best CTC path WHOSE COLLAPSED STRING CONTAINS THE ENTRY AS A SUBSTRING
//             over the best unconstrained path; <= 0.  No expf or logf is involved anywhere;
//   states    s = 0 .. 2 L - 2: an even s is token k[s / 2], an odd s the blank between two tokens (cls_of()).  There is no
//             leading or trailing blank state: those frames are filler.  skip(s) holds when s is even, s >= 2 and k[s / 2] differs
//             from k[s / 2 - 1] (skip_of()).  Each state carries (v, a): its value and the frame its segment started at (Cell);
//   t = 0     state 0 is (d[0][k[0]], 0), every other state (-inf, -1);
//   t >= 1    state 0: best = its own (v, a) of step t - 1, replaced by (0, t) unless v >= 0 -- a tie keeps the earlier start, a
//             NaN restarts.  State s >= 1: best = its own, replaced by state s - 1's only when that is strictly greater, then,
//             where skip(s), by state s - 2's only when that is strictly greater.  New v = d[t][cls(s)] + best.v, new a = best.a
//             (step());
//   end       after every step the value of state 2 L - 2 is a candidate for the entry's result (score, first_col = a, last_col
//             = t); it replaces the running result only when strictly greater: the earliest end wins;
//   feasible  an entry with T < lx::need_of(k) ends at -inf, span (-1, -1), and is never a hit;
//   hits      of a line: the entries with score > -inf and score >= min_score (a NaN never passes), up to HITS of them ordered
//             by score descending, then entry index ascending (cc::better), each as (entry, score, first_col, last_col).
// Scope: one occurrence per (line, entry), the best.  Several occurrences, length normalisation and whole-word matching are out
// of scope.  Lines of list 0 (none) take no part: no row of theirs is gathered, no launch sees them, no value of theirs is
// written.  Sharing the recomputed logits with a lexicon on the same line is out of scope too.
#pragma once
#include <math.h>
#include <stdint.h>

#include "ctc_lexicon.h"
#include "word_boxes.h"

namespace rt {
namespace kw {

constexpr int MAX_LISTS = 16;   // RT_MAX_KEYWORD_LISTS
constexpr int HITS = 8;         // RT_KEYWORD_HITS

// one hit; the same layout as rt_keyword_hit (include/retto_hip.h).  quad: the span's page quad, filled on the host by results()
// (session.cpp); the kernels and the debug hooks never touch it
struct Hit { int32_t entry; float score; int32_t first_col, last_col; float quad[8]; };
// one line that carries a list: lx::Line with lex = the 0-based list, out = the first slot of its score row
using Line = lx::Line;
// a state's value and the frame its segment started at
struct Cell { float v; int32_t a; };

// the class of state s of an entry of L ids (2 L - 1 states)
RT_HD int cls_of(const int32_t* ids, int s) { return (s & 1) ? 0 : ids[s >> 1]; }
RT_HD bool skip_of(const int32_t* ids, int s) { return !(s & 1) && s >= 2 && ids[s >> 1] != ids[(s >> 1) - 1]; }
// state s at step t >= 1 from the cells of step t - 1: its own, state s - 1's and state s - 2's (read only where s >= 1 / skip)
// and d = l[t][cls(s)] - rmax[t]
RT_HD Cell step(int s, int t, Cell own, Cell p1, Cell p2, bool skip, float d) {
  Cell best = own;
  if (s == 0) {
    if (!(best.v >= 0.0f)) best = Cell{0.0f, t};
  } else {
    if (p1.v > best.v) best = p1;
    if (skip && p2.v > best.v) best = p2;
  }
  return Cell{d + best.v, best.a};
}
// a hit passes the list's threshold
RT_HD bool passes(float score, float min_score) { return score > -INFINITY && score >= min_score; }

// Host only: the page quad (after-resize_both coordinates; the caller applies gm::scale_and_clip) of a hit's span [first_col,
// last_col + 1), exactly as wb::line_words maps an ALNUM word's columns: crop pixels per column, then wb::span_to_quad
inline void span_quad(int first_col, int last_col, const wb::WordGeom& g, int rot180, float* q) {
  if (g.T <= 0 || g.resized_w <= 0) { for (int i = 0; i < 8; i++) q[i] = 0.0f; return; }
  const float p = ((float)g.W / (float)g.T) * ((float)g.w_c / (float)g.resized_w);   // crop pixels per column
  wb::span_to_quad((float)first_col * p, (float)(last_col + 1) * p, g, rot180, q);
}

// Host reference, plain fp32 loops: the row maximum of one row of logits [N], by k_ctc_row_max's comparison
inline float row_max(const float* logits, int N) {
  float mx = -INFINITY;
  for (int c = 0; c < N; c++) if (logits[c] > mx) mx = logits[c];
  return mx;
}
// Host reference: the result of one entry (ids [L]) over a line's logits [T][ld] and rmax [T] -> its score; span[0..2) = its
// first and last column, (-1, -1) with a score of -inf
inline float entry_spot(const float* logits, int ld, const float* rmax, int T, const int32_t* ids, int L, int32_t* span) {
  span[0] = span[1] = -1;
  if (T < lx::need_of(ids, L)) return -INFINITY;
  const int S = 2 * L - 1;
  Cell a[2 * lx::MAX_LEN - 1], b[2 * lx::MAX_LEN - 1];
  float score = -INFINITY;
  for (int t = 0; t < T; t++) {
    for (int s = 0; s < S; s++) {
      const float d = logits[(size_t)t * ld + cls_of(ids, s)] - rmax[t];
      if (t == 0) b[s] = s == 0 ? Cell{d, 0} : Cell{-INFINITY, -1};
      else b[s] = step(s, t, a[s], s >= 1 ? a[s - 1] : Cell{-INFINITY, -1}, s >= 2 ? a[s - 2] : Cell{-INFINITY, -1}, skip_of(ids, s), d);
    }
    for (int s = 0; s < S; s++) a[s] = b[s];
    if (a[S - 1].v > score) { score = a[S - 1].v; span[0] = a[S - 1].a; span[1] = t; }
  }
  return score;
}
// Host reference: the hits of one line from its score row [n] and spans [n][2]; writes entry, score and the columns of up to HITS
// hits (never a quad) and returns their number
inline int line_hits(const float* score, const int32_t* span, int n, float min_score, Hit* out) {
  float L[HITS]; int I[HITS];
  for (int j = 0; j < HITS; j++) { L[j] = -INFINITY; I[j] = cc::EMPTY_ID; }
  for (int e = 0; e < n; e++)
    if (passes(score[e], min_score)) cc::list_insert(L, I, score[e], e);
  int cnt = 0;
  for (int j = 0; j < HITS && I[j] != cc::EMPTY_ID; j++) {
    Hit& h = out[cnt++];
    h.entry = I[j]; h.score = L[j]; h.first_col = span[2 * (size_t)I[j]]; h.last_col = span[2 * (size_t)I[j] + 1];
  }
  return cnt;
}

}  // namespace kw
}  // namespace rt
