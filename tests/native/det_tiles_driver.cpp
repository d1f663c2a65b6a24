// Host-only driver for the det tile plan (retto_amd/csrc/det_tiles.h), compiled with g++ -fsanitize=address,undefined by
// tests/test_det_tiles_cpu.py and run as a program: no GPU, nothing loaded into Python.  One query per input line:
//   L T O          the plan along one axis of length L
//   page H W T O   the checks of a whole det input
// One answer line each:
//   n=.. len=.. x=a,b,.. b=a,b,..      or      invalid: <what is wrong>      or      page: <status> tiled=<0|1>
// The plan's own properties (partition, tiles inside the page, boundaries O / 2 inside both tiles and multiples of 16) are
// checked here too, through the per-index functions a kernel would call; a violation ends the program with status 2.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "det_tiles.h"

using namespace rt;

static int fail(const char* what, int L, int T, int O, int i) {
  fprintf(stderr, "det_tiles_driver: %s at L=%d T=%d O=%d i=%d\n", what, L, T, O, i);
  return 2;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    if (line.rfind("page", 0) == 0) {
      std::string word; int H, W, T, O;
      in >> word >> H >> W >> T >> O;
      if (!in) { printf("bad query\n"); continue; }
      if (const char* why = dt::check_params(T, O)) { printf("invalid: %s\n", why); continue; }
      std::string why;
      const int rc = dt::check_page(H, W, &why);
      printf("page: %d tiled=%d\n", rc, rc == dt::OK && dt::page_tiled(H, W, T) ? 1 : 0);
      continue;
    }
    int L, T, O;
    in >> L >> T >> O;
    if (!in) { printf("bad query\n"); continue; }
    if (const char* why = dt::check_params(T, O)) { printf("invalid: %s\n", why); continue; }
    const dt::Axis a = dt::axis_plan(L, T, O);
    const int n = a.n();
    if (n != dt::axis_tiles(L, T, O) || a.len != dt::axis_tile_len(L, T)) return fail("count", L, T, O, 0);
    for (int i = 0; i < n; i++) {
      const int x = a.origin[(size_t)i], b = a.bound[(size_t)i], lo = a.own0(i);
      if (x != dt::axis_origin(L, T, O, i) || b != dt::axis_bound(L, T, O, i) || lo != dt::axis_bound(L, T, O, i - 1)) return fail("per-index form", L, T, O, i);
      if (x < 0 || x + a.len > L) return fail("tile outside the page", L, T, O, i);
      if (!(lo < b) || lo < x || b > x + a.len) return fail("ownership outside the tile", L, T, O, i);
      if (b % 16 != 0) return fail("boundary alignment", L, T, O, i);
      if (i + 1 < n && (b - a.origin[(size_t)i + 1] < O / 2 || x + a.len - b < O / 2)) return fail("boundary too close to a tile edge", L, T, O, i);
    }
    if (a.bound[(size_t)n - 1] != L) return fail("partition", L, T, O, n - 1);
    printf("n=%d len=%d x=", n, a.len);
    for (int i = 0; i < n; i++) printf("%s%d", i ? "," : "", a.origin[(size_t)i]);
    printf(" b=");
    for (int i = 0; i < n; i++) printf("%s%d", i ? "," : "", a.bound[(size_t)i]);
    printf("\n");
  }
  return 0;
}
