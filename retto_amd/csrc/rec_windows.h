// Rec windows: the recogniser run over overlapping windows of a long line, written once for the session (rec_groups: session.cpp),
// the two data-movement kernels (k_rec_window_cut, k_rec_window_stitch: prepost_kernels.hip), rt_rec_window_plan and the CPU check
// (tests/native/rec_windows_driver.cpp).  A line far wider than anything the rec network was trained at -- a text line across a
// 7680-pixel scan is a 48 x 3000 tensor with 400 time steps -- is cut into units of one fixed width; the network runs on the
// units as its "lines", and each unit's trusted time steps are copied into the ONE line's rows of (idx, prob) and head-input
// features z5 that the CTC tail reads.  Nothing downstream changes: the line keeps its T, its width and its geometry, so the
// greedy decode, word boxes, candidates, charsets, lexicons, patterns, keywords and beams read a long line as they read any
// other.  The reference has no counterpart; the rule here is this project's own.  This header needs no HIP header, so a
// stand-alone program can include it.
//
// Units.  A rec tensor is 48 x L pixels and has T(L) = tokens(L) time steps (RecNet::tokens_for_width: two stride-2 stages and
// a pool of 2).  One time step is 8 pixel columns: step j covers the columns [8j, 8j + 8); a trailing partial step is dropped
// (up to L mod 8 = 4; from 5 on the strides' round-up makes it one more step).
//
// The plan along a line of width L, for window W and overlap O.  last = floor8(L - W), rounded down to a multiple of 8.
//   W = 0 or last <= 0   the line is whole: one unit [0, L), today's path.  This covers every L < W + 8.
//   otherwise            S = W - O, n = ceil(last / S) + 1 units at origins x_i = min(i S, last).  Units 0 .. n - 2 are W wide,
//                        the last one L - x_{n-1} = W + L mod 8.  Every origin is a multiple of 8, so the three stride-2 stages
//                        and the pool keep their phase: unit i's step k is the line's step x_i / 8 + k, and the last unit ends
//                        exactly at the line's last step, x_{n-1} / 8 + T(width_{n-1}) = T(L).
// Ownership, in steps.  m_i = x_i / 8, Tw = W / 8.  c_-1 = 0, c_i = (m_i + Tw + m_{i+1}) / 2 for i < n - 1 (the middle of the
// pair's overlap), c_{n-1} = T(L); step t belongs to the one unit i with c_{i-1} <= t < c_i, at row t - m_i of that unit.  An
// interior boundary lies at least O / 16 steps inside both units of its pair: the outer half of a unit's overlap, where its
// truncated glyphs and the zero padding of the convolutions act, is discarded.
// The stitch is a selection,
//   line_row[t] = unit_row(i(t))[t - m_i]
// for the idx row, the prob row and the 120-float z5 row alike: every line row is written once and the order of the units does
// not matter.
//
// Parameters.  W = 0 is off.  Otherwise W is a multiple of 32 with W >= MIN_WINDOW, O a multiple of 32 with 0 <= O <= W / 2 (so
// the stride is at least W / 2).  check_params() names the parameter.
//
// What is not claimed: that windows read long lines better.  The effect on accuracy with trained weights has not been measured.
#pragma once
#include <cstdint>
#include <vector>

namespace rt {
namespace rw {

constexpr int STEP = 8;          // pixel columns per time step
constexpr int CELL = 32;         // what the window and the overlap are a multiple of
constexpr int MIN_WINDOW = 128;
constexpr int Z5_D = 120;        // floats of a z5 row (SvtrCore::D): 30 float4

// nullptr when (window, overlap) is accepted, else what is wrong with which parameter
inline const char* check_params(int window, int overlap) {
  if (window < 0) return "window is negative";
  if (window == 0) return overlap < 0 ? "overlap is negative" : nullptr;   // off: the overlap is kept and not read
  if (window % CELL != 0) return "window must be 0 (off) or a multiple of 32";
  if (window < MIN_WINDOW) return "window must be 0 (off) or at least 128";
  if (overlap < 0) return "overlap is negative";
  if (overlap % CELL != 0) return "overlap must be a multiple of 32";
  if (overlap > window / 2) return "overlap must be at most window / 2";
  return nullptr;
}

// T(L): RecNet::tokens_for_width, restated here so that the header stands alone (session.cpp asserts that the two agree)
inline int tokens(int L) {
  const int wa = (L - 1) / 2 + 1, wc = (wa - 1) / 2 + 1;
  return wc >= 2 ? (wc - 2) / 2 + 1 : 0;
}
// floor8(L - W); only read where it is positive
inline int last_origin(int L, int W) { return L - W >= STEP ? (L - W) / STEP * STEP : 0; }
// a line is read in windows when windows are on and it is at least 8 columns wider than one
inline bool line_windowed(int L, int W) { return W > 0 && last_origin(L, W) > 0; }
// units of a line
inline int units(int L, int W, int O) {
  if (!line_windowed(L, W)) return 1;
  const int S = W - O;
  return (last_origin(L, W) + S - 1) / S + 1;
}
// x_i, 0 <= i < units
inline int origin(int L, int W, int O, int i) {
  if (!line_windowed(L, W)) return 0;
  const long long x = (long long)i * (W - O);
  const int last = last_origin(L, W);
  return x < last ? (int)x : last;
}
// width of unit i
inline int width(int L, int W, int O, int i) {
  if (!line_windowed(L, W)) return L;
  return i < units(L, W, O) - 1 ? W : L - last_origin(L, W);
}
// c_i, -1 <= i < units
inline int bound(int L, int W, int O, int i) {
  if (i < 0) return 0;
  if (i >= units(L, W, O) - 1) return tokens(L);
  return (origin(L, W, O, i) / STEP + W / STEP + origin(L, W, O, i + 1) / STEP) / 2;
}
// pixel columns of all units of a line: what the line costs a launch group
inline long long unit_columns(int L, int W, int O) {
  if (!line_windowed(L, W)) return L;
  return (long long)(units(L, W, O) - 1) * W + (L - last_origin(L, W));
}

struct Plan {
  int T = 0;                               // the line's time steps
  std::vector<int> origin, width, bound;   // [n] each; unit i owns the steps [i ? bound[i - 1] : 0, bound[i])
  int n() const { return (int)origin.size(); }
  int own0(int i) const { return i ? bound[(size_t)i - 1] : 0; }
};
inline Plan plan(int L, int W, int O) {
  Plan p;
  p.T = tokens(L);
  const int n = units(L, W, O);
  p.origin.resize((size_t)n); p.width.resize((size_t)n); p.bound.resize((size_t)n);
  for (int i = 0; i < n; i++) {
    p.origin[(size_t)i] = origin(L, W, O, i); p.width[(size_t)i] = width(L, W, O, i); p.bound[(size_t)i] = bound(L, W, O, i);
  }
  return p;
}

// One unit of a rec group as the two kernels read it.  cut: the columns [x0, x0 + w) of the 48 rows of the line tensor at
// lines + src_off (line_w float4 a row) -> 48 x w float4, contiguous, at units + dst_off.  stitch: the line's steps [t0, t1),
// rows [t0 - m, t1 - m) of the unit's rows from unit_row on -> rows [t0, t1) of the line's rows from line_row on.
struct UnitDesc {
  long long src_off, dst_off;     // float4 (one NHWC-4 pixel)
  long long unit_row, line_row;   // rows
  int line_w, x0, w;
  int m, t0, t1;
};

}  // namespace rw
}  // namespace rt
