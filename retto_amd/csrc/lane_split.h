// How a batch's pages go over the session's lanes: how many lanes a call of n pages uses, and which contiguous range of pages
// each of them gets.  Plain C++ as det_tiles.h and rec_line_opts.h: no HIP; built and checked without a GPU
// (tests/test_lane_split_cpu.py).
#pragma once
#include <algorithm>
#include <vector>

namespace rt {

// The lanes of a call over n_pages pages: the session's, at most `active` of them (rt_set_lanes), at most one per page, at least 1.
inline int lanes_for(int lanes, int active, int n_pages) { return std::max(1, std::min(std::min(lanes, active), std::max(n_pages, 1))); }

// first[l] .. first[l + 1] = the pages of lane l of nl, nl + 1 entries: contiguous ranges of about equal work, order preserved.
// A page's work: its det pixels after the session size limit (a2) plus a constant for its lines; equal page counts when the pages
// are all one size.  No range is empty while n_pages >= nl.
inline std::vector<int> lane_split(const int* hs, const int* ws, int n_pages, int max_side_len, int nl) {
  std::vector<int> first((size_t)nl + 1, 0);
  std::vector<double> cost((size_t)n_pages);
  double total = 0;
  for (int i = 0; i < n_pages; i++) {
    const double h = std::max(hs[i], 1), w = std::max(ws[i], 1);
    const double r = std::min(1.0, (double)max_side_len / std::max(h, w));
    total += cost[(size_t)i] = h * w * r * r + 250000.0;
  }
  double acc = 0;
  int l = 1;
  for (int i = 0; i < n_pages && l < nl; i++) {
    acc += cost[(size_t)i];
    // close range l-1 after page i once its share is reached, leaving at least one page for each later lane
    if (acc >= total * l / nl - 1e-6 || n_pages - (i + 1) <= nl - l) first[(size_t)l++] = i + 1;  // one range per page: none empty
  }
  for (; l <= nl; l++) first[(size_t)l] = n_pages;
  for (int k = 1; k <= nl; k++) first[(size_t)k] = std::max(first[(size_t)k], first[(size_t)k - 1]);
  return first;
}

}  // namespace rt
