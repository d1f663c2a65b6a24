// Rec flip: a line the angle classifier is unsure of is read both ways up, and the better reading is kept.  Written once for
// the session (rec_groups: session.cpp), the two data-movement kernels (k_rec_flip_rotate, k_rec_flip_select:
// prepost_kernels.hip), rt_rec_flip_choose and the CPU check (tests/native/rec_flip_driver.cpp).  Whether a line is upside down
// is decided by the small mobile classifier and one fixed threshold (cls_thresh, k_cls_post_rotate): a line labelled 180 at
// score 0.7 is not rotated, a line wrongly labelled 0 stays upside down, and rt_run_regions callers hand in quads in any corner
// order.  An upside-down line is garbage for every rec option, and none can repair it: they all read the same rows.  The usual
// remedy in PP-OCR deployments is to let the recogniser decide; the reference has no counterpart, the rule here is this
// project's own.  Needs no HIP header beyond geom_math.h's RT_HD, so a stand-alone program can include it.
//
// Setting.  rt_set_rec_flip(s, cls_below), per session.  cls_below = 0: off, the initial state.  Otherwise a line is read both
// ways iff its classifier score -- rt_results_cls_scores, the score of the argmax label -- is below cls_below (an fp32 <);
// any value above 1 reads every line both ways.  NaN, a negative value or an infinity: RT_ERR_INVALID naming the parameter.
// With 0 < cls_below <= 1 the pipeline needs the classifier scores on the host between the cls stage and the rec plan: one
// copy of one float per line and ONE LANE SYNC per call, only then.  Above 1 no sync is added.
//
// Two views of a both-ways line.  View 0 is the crop as the cls stage left it.  View 1 is that crop rotated by 180 degrees,
// pixel (y, x) -> (h - 1 - y, w - 1 - x): what k_cls_post_rotate does, and in a row-major crop of n = h * w pixels simply pixel
// p -> n - 1 - p.  Both go through the same resize_norm at the same padded width W that the rec plan gave the line.  The
// thumbnail arithmetic is not rotation-symmetric (its bounds are ceils), so view 1 is resize_norm of the ROTATED CROP, not a
// rotation of the normalised tensor: k_rec_flip_rotate copies the flagged crops rotated into a second pool region and the
// existing k_resize_norm reads that region.  A rotation by 180 degrees keeps a line's rec width and its number of time steps.
//
// One pass.  A rec group's tensor is its lines followed by the view-1 copies of its both-ways lines; the network runs once over
// that list (rec windows apply to each view as to any line), a both-ways line is charged twice in the group's pixel budget.
//
// Scores.  Each view gets the greedy CTC score by k_ctc_decode itself over that view's rows: the kept count, a sequential fp32
// sum of the kept probabilities in step order, one division (0 / 0 = NaN for a view that kept nothing).
//
// Choice (choose()).  View 1 is taken iff it kept at least one token, and either view 0 kept none or score1 > score0 (fp32).  A
// tie or a NaN keeps view 0.  Charsets, snap and patterns act after the choice, on the chosen rows.
//
// Selection.  The chosen view's rows -- idx, prob, and the 120-float z5 row when the tail needs it -- become the line's rows, by
// copy; every row of a line comes from one view, nothing is recomputed.  (The views' rows lie in scratch, view 0 of every line
// first, in line order: that prefix is the lines' row layout, so one block copy brings every line's view-0 idx / prob rows to
// the line rows and the z5 prefix IS the lines' z5.  k_rec_flip_select then copies the chosen view's rows of the both-ways
// lines over them -- z5 only where view 1 is taken, a kept view 0 being in place -- and copies nothing for any other line.)
//
// Orientation downstream.  The line's effective 180 rotation is (the classifier rotated it) XOR (view 1 taken): word boxes and
// keyword span quads use that as their rot180.  rt_results_cls_labels / cls_scores stay the classifier's own outputs.
//
// Nothing reads the crop pool after rec_groups, so the winners' crops are not rotated in place.
//
// Out of scope: a per-region flip flag; 90 / 270 degree views; switching the classifier off; choosing by anything but the
// greedy score; flipping in rt_rec, rt_rec_ragged or rt_ctc_decode.
// What is not claimed: that flipping reads real lines better.  The weights here are synthetic; the effect on accuracy with
// trained PP-OCRv4 weights has not been measured.
#pragma once
#include <cstdint>
#include "geom_math.h"

namespace rt {
namespace rf {

// outcome of a line (rt_results_rec_flip)
constexpr int ONE_WAY = 0, KEPT_0 = 1, TOOK_1 = 2;

// nullptr when cls_below is accepted, else what is wrong with it (x == x && x - x == 0: neither NaN nor an infinity)
inline const char* check_param(float cls_below) {
  if (!(cls_below == cls_below)) return "cls_below is NaN";
  if (cls_below < 0.0f) return "cls_below is negative";
  if (!(cls_below - cls_below == 0.0f)) return "cls_below is infinite";
  return nullptr;
}
// every line is read both ways whatever its score: no score has to reach the host
RT_HD bool every_line(float cls_below) { return cls_below > 1.0f; }
// the host needs the classifier scores before the rec plan
RT_HD bool needs_scores(float cls_below) { return cls_below > 0.0f && !every_line(cls_below); }
// is a line of classifier score cls_score read both ways?
RT_HD bool both_ways(float cls_score, float cls_below) {
  if (!(cls_below > 0.0f)) return false;
  return every_line(cls_below) || cls_score < cls_below;
}
// the choice between the two views' (kept tokens, greedy score): 1 = view 1 is taken
RT_HD int choose(int ntok0, float score0, int ntok1, float score1) {
  if (ntok1 <= 0) return 0;
  if (ntok0 <= 0) return 1;
  return score1 > score0 ? 1 : 0;
}
// the effective 180 rotation of a line
RT_HD int rot180(int cls_rotated, int outcome) { return (cls_rotated ? 1 : 0) ^ (outcome == TOOK_1 ? 1 : 0); }

// ---- k_rec_flip_rotate: the flagged crops as one flat list of pixels -----------------------------------------------------
// Crop c has npix = h * w pixels of 3 bytes at src_off in the crop pool, its rotated copy at dst_off in the second region;
// pix_base = the pixels of the crops before it (every crop has at least one pixel, so the bases strictly increase).  Pixel g of
// the list belongs to the last crop whose pix_base <= g.
struct FlipCrop { long long src_off, dst_off, pix_base, npix; };
RT_HD int find_crop(const FlipCrop* crops, int n, long long g) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (crops[mid].pix_base <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// destination pixel p of a crop of npix pixels is its source pixel npix - 1 - p: (y, x) <- (h - 1 - y, w - 1 - x)
RT_HD long long src_pixel(long long npix, long long p) { return npix - 1 - p; }

// ---- k_rec_flip_select: one both-ways line of a rec group ---------------------------------------------------------------
// v0 / v1: the two views' indices in the group's view list (what k_ctc_decode's counts and scores are indexed by); row0 / row1:
// their first rows in the views' idx / prob / z5; out_row: the line's first row in the line rows; T: its time steps; slot: the
// line's index in the per-call outcome and score arrays.
struct SelectDesc { long long row0, row1, out_row; int v0, v1, T, slot; };

}  // namespace rf
}  // namespace rt
