// Rec lexicons: a caller's word list ranked by CTC likelihood per line (rt_lexicon_create, rt_set_rec_lexicon,
// rt_run_regions_lexicons), written once for the device kernels (k_ctc_row_lse, k_ctc_lexicon_forward, k_ctc_lexicon_topk:
// prepost_kernels.hip) and the CPU check (rt_debug_ctc_lexicon_host).  For the enumerated field: the region holds one of N known
// strings.  A charset only narrows the alphabet, candidates only exist at the time steps the greedy decode kept, and matching the
// greedy text against the list afterwards throws the model's probabilities away.  The reference has no counterpart: the rule here
// is this project's own.
//
// A lexicon is an ordered list of entries; entry e is a sequence of L_e class ids, 1 <= L_e <= MAX_LEN, never the blank 0; equal
// neighbours are allowed.  For a line of T time steps that carries a lexicon:
//   l[t][c]   the RECOMPUTED fp32 logit sum_k z5[row][k] * W[k][c] + b[c], exactly what the candidates and charsets paths compute;
//   lse[t]    log-sum-exp over every class c < classes (lse_of(): mx + logf(sum_c expf(l - mx))); the GEMM's pad columns
//             [classes, round_up(classes, 4)) take no part;
//   lp[t][c]  l[t][c] - lse[t]: the FULL softmax -- not restricted to the lexicon's alphabet, nor to the line's charset if it has
//             one.  A charset changes the decode; a lexicon reads the model's own distribution.
//   states    the extended sequence has S = 2 L + 1 states: even states are the blank, odd state s is token (s - 1) / 2 (cls_of());
//   forward   in the log domain, fp32: alpha_0[0] = lp[0][0], alpha_0[1] = lp[0][token 0], the rest -inf; for t >= 1
//             alpha_t[s] = lae(alpha_{t-1}[s], alpha_{t-1}[s-1], skip ? alpha_{t-1}[s-2] : -inf) + lp[t][cls(s)]  (step()), where
//             skip holds when s is odd, s >= 3 and token (s-1)/2 differs from token (s-3)/2 (skip_of()); a state below 0 is -inf;
//   loglik    lae(alpha_{T-1}[S-1], alpha_{T-1}[S-2], -inf);
//   lae       m = the max of its arguments; -inf if m is -inf, otherwise m + logf(sum of expf(x - m)) in argument order;
//   feasible  entry e is feasible for T when T >= need(e) = L_e + (number of equal-neighbour pairs in e); otherwise its loglik is
//             -inf and it is never reported;
//   result    up to MATCHES feasible entries ordered by loglik descending, then entry index ascending (cc::better), each as
//             (entry, loglik, posterior), posterior = expf(loglik - LSE over the line's feasible entries) (posterior_of()).
//             Fewer feasible entries give fewer matches, none gives 0.
// Everything else of the line -- tokens, score, text, word boxes, candidates, JSON -- is what it is without the lexicon, bit for
// bit: nothing here writes a value the decode reads.  Out of scope here; the Viterbi alignment of the winner, and replacing the
// line's decode by it where the caller switched that on (rt_lexicon_set_snap), live in ctc_lexicon_align.h.  Lines of lexicon 0
// (none) take no part: no row of theirs is gathered, no launch sees them, no value of theirs is written.
//
// Device layout (Tables).  Entries of all lexicons sit in one flat list; lexicon k (0-based) owns entries [first, first + n).
// At create time a lexicon's entries are bucketed by length into lane widths -- 16 lanes (L <= 7, S <= 15), 32 lanes (L <= 15),
// 64 lanes (L <= 31, S <= 63) -- and `order` lists them bucket by bucket, by entry index within a bucket; a wave of the forward
// kernel carries 4 / 2 / 1 entries of one bucket of one line, one lane per state.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "ctc_candidates.h"

namespace rt {
namespace lx {

constexpr int MAX_LEXICONS = 16;      // RT_MAX_LEXICONS
constexpr int MAX_ENTRIES = 65536;    // RT_LEXICON_MAX_ENTRIES
constexpr int MAX_LEN = 31;           // RT_LEXICON_MAX_LEN
constexpr int MATCHES = 4;            // RT_LEXICON_MATCHES
constexpr int LINES_PER_CHUNK = 4096; // (a chunk's lines are one grid dimension of the forward kernel)
// The loglik table of one rec group (one float per entry of the lexicon of each of its lexicon lines) lives in the scratch arena
// until the group's top-K has run; a group that would need more fails with RT_ERR_CAPACITY naming the lexicons (256 MB: 1024
// lines of a 65536-entry lexicon).  Splitting the table with the lines is the way to lift it.
constexpr long long MAX_GROUP_TABLE = 1ll << 26;

// one match; the same layout as rt_lexicon_match (include/retto_hip.h)
struct Match { int32_t entry; float loglik; float posterior; };
// one entry of the flat list: its ids at ids[off ..], their number, and the fewest time steps it needs
struct Entry { int32_t off, len, need; };
// one lexicon: its entries [first, first + n) of the flat list (and of `order`), n16 / n32 of them in the 16- / 32-lane buckets
struct Lex { int32_t first, n, n16, n32; };
// one line that carries a lexicon: its T rows start at position row0 of the call's compact row list, lex is 0-based, its
// loglik row starts at loglik[out], its matches go to matches[slot * MATCHES ...] and counts[slot]
struct Line { int32_t row0, T, lex, slot; long long out; };

RT_HD int width_of(int L) { return L <= 7 ? 16 : L <= 15 ? 32 : 64; }
RT_HD int waves_of(const Lex& x) { return (x.n16 + 3) / 4 + (x.n32 + 1) / 2 + (x.n - x.n16 - x.n32); }
// the class of state s of an entry of L ids (S = 2 L + 1 states)
RT_HD int cls_of(const int32_t* ids, int s) { return (s & 1) ? ids[(s - 1) >> 1] : 0; }
RT_HD bool skip_of(const int32_t* ids, int s) { return (s & 1) && s >= 3 && ids[(s - 1) >> 1] != ids[(s - 3) >> 1]; }
RT_HD int need_of(const int32_t* ids, int L) {
  int n = L;
  for (int i = 1; i < L; i++) n += ids[i] == ids[i - 1] ? 1 : 0;
  return n;
}
RT_HD float lae(float a, float b, float c) {
  const float m = fmaxf(fmaxf(a, b), c);
  if (m == -INFINITY) return -INFINITY;
  return m + logf(expf(a - m) + expf(b - m) + expf(c - m));
}
RT_HD float lse_of(float mx, float sum) { return mx + logf(sum); }
// alpha_t[s] from alpha_{t-1}[s], [s-1], [s-2] (callers pass -inf for a state below 0) and lp = l[t][cls(s)] - lse[t]
RT_HD float step(float a0, float a1, float a2, bool skip, float lp) { return lae(a0, a1, skip ? a2 : -INFINITY) + lp; }
RT_HD float posterior_of(float loglik, float mx, float sum) { return expf(loglik - lse_of(mx, sum)); }

// The device tables of a list of lexicons, built on the host (build()): what rt_lexicon_create stores and the debug hook makes
struct Tables {
  std::vector<int32_t> ids;      // every entry's ids, entry after entry
  std::vector<Entry> entries;    // the flat entry list
  std::vector<int32_t> order;    // per lexicon at [first, first + n): its entries (lexicon-local indices) bucket by bucket
  std::vector<Lex> lex;
  void clear() { ids.clear(); entries.clear(); order.clear(); lex.clear(); }
  // appends one lexicon of n entries (entry i: lens[i] ids, consecutive in e_ids)
  void add(const int32_t* e_ids, const int32_t* lens, int n) {
    Lex x{(int32_t)entries.size(), n, 0, 0};
    size_t o = 0;
    for (int i = 0; i < n; i++) {
      entries.push_back(Entry{(int32_t)ids.size(), lens[i], need_of(e_ids + o, lens[i])});
      ids.insert(ids.end(), e_ids + o, e_ids + o + lens[i]);
      o += (size_t)lens[i];
    }
    for (int w = 16; w <= 64; w *= 2)
      for (int i = 0; i < n; i++)
        if (width_of(lens[i]) == w) { order.push_back(i); if (w == 16) x.n16++; else if (w == 32) x.n32++; }
    lex.push_back(x);
  }
};
// the four tables on the device (pt::DevTables' counterpart)
struct DevTables { const int32_t* ids; const Entry* entries; const int32_t* order; const Lex* lex; };

// Host reference, plain fp32 loops: lse of one row of logits [N]
inline float row_lse(const float* logits, int N) {
  float mx = -INFINITY;
  for (int c = 0; c < N; c++) if (logits[c] > mx) mx = logits[c];
  float sum = 0.0f;
  for (int c = 0; c < N; c++) sum = sum + expf(logits[c] - mx);
  return lse_of(mx, sum);
}
// Host reference: the log-likelihood of one entry (ids [L]) over a line's logits [T][ld] and lse [T]
inline float entry_loglik(const float* logits, int ld, const float* lse, int T, const int32_t* ids, int L) {
  if (T < need_of(ids, L)) return -INFINITY;
  const int S = 2 * L + 1;
  float a[2 * MAX_LEN + 1], b[2 * MAX_LEN + 1];
  for (int s = 0; s < S; s++) a[s] = s < 2 ? logits[cls_of(ids, s)] - lse[0] : -INFINITY;
  for (int t = 1; t < T; t++) {
    for (int s = 0; s < S; s++)
      b[s] = step(a[s], s >= 1 ? a[s - 1] : -INFINITY, s >= 2 ? a[s - 2] : -INFINITY, skip_of(ids, s),
                  logits[(size_t)t * ld + cls_of(ids, s)] - lse[t]);
    for (int s = 0; s < S; s++) a[s] = b[s];
  }
  return lae(a[S - 1], a[S - 2], -INFINITY);
}
// Host reference: the matches of one line from its loglik row [n]; returns their number
inline int line_matches(const float* loglik, int n, Match* out) {
  float L[MATCHES]; int I[MATCHES];
  for (int j = 0; j < MATCHES; j++) { L[j] = -INFINITY; I[j] = cc::EMPTY_ID; }
  float mx = -INFINITY;
  for (int e = 0; e < n; e++)
    if (loglik[e] > -INFINITY) { mx = fmaxf(mx, loglik[e]); cc::list_insert(L, I, loglik[e], e); }
  float sum = 0.0f;
  for (int e = 0; e < n; e++)
    if (loglik[e] > -INFINITY) sum = sum + expf(loglik[e] - mx);
  int cnt = 0;
  for (int j = 0; j < MATCHES && I[j] != cc::EMPTY_ID; j++) out[cnt++] = Match{I[j], L[j], posterior_of(L[j], mx, sum)};
  return cnt;
}

}  // namespace lx
}  // namespace rt
