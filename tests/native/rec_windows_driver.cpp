// Host-only driver for the rec window plan (retto_amd/csrc/rec_windows.h), compiled with g++ -fsanitize=address,undefined by
// tests/test_rec_windows_cpu.py and run as a program: no GPU, nothing loaded into Python.  One query per input line:
//   L W O          the plan of a line of L columns for window W and overlap O
// One answer line each:
//   n=.. T=.. x=a,b,.. w=a,b,.. c=a,b,..      or      invalid: <what is wrong>
// The plan's own properties (units inside the line, the last unit ends at the line's last step, ownership inside the unit, the
// intervals partition [0, T), boundaries O / 16 steps inside both units) are checked here too, through the per-index functions;
// a violation ends the program with status 2.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "rec_windows.h"

using namespace rt;

static int fail(const char* what, int L, int W, int O, int i) {
  fprintf(stderr, "rec_windows_driver: %s at L=%d W=%d O=%d i=%d\n", what, L, W, O, i);
  return 2;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    int L, W, O;
    in >> L >> W >> O;
    if (!in) { printf("bad query\n"); continue; }
    if (const char* why = rw::check_params(W, O)) { printf("invalid: %s\n", why); continue; }
    const rw::Plan p = rw::plan(L, W, O);
    const int n = p.n();
    if (n != rw::units(L, W, O) || p.T != rw::tokens(L)) return fail("count", L, W, O, 0);
    if ((n > 1) != rw::line_windowed(L, W)) return fail("windowed", L, W, O, 0);
    long long cols = 0;
    for (int i = 0; i < n; i++) {
      const int x = p.origin[(size_t)i], w = p.width[(size_t)i], c = p.bound[(size_t)i], lo = p.own0(i), m = x / rw::STEP;
      if (x != rw::origin(L, W, O, i) || w != rw::width(L, W, O, i) || c != rw::bound(L, W, O, i) || lo != rw::bound(L, W, O, i - 1))
        return fail("per-index form", L, W, O, i);
      if (x < 0 || x % rw::STEP != 0 || w < rw::STEP || x + w > L) return fail("unit outside the line", L, W, O, i);
      if (!(lo < c) || lo < m || c > m + rw::tokens(w)) return fail("ownership outside the unit", L, W, O, i);
      if (i + 1 < n && (c - p.origin[(size_t)i + 1] / rw::STEP < O / 16 || m + W / rw::STEP - c < O / 16))
        return fail("boundary too close to a unit edge", L, W, O, i);
      cols += w;
    }
    if (p.bound[(size_t)n - 1] != p.T) return fail("partition", L, W, O, n - 1);
    if (p.origin[(size_t)n - 1] / rw::STEP + rw::tokens(p.width[(size_t)n - 1]) != p.T) return fail("the last unit's end", L, W, O, n - 1);
    if (cols != rw::unit_columns(L, W, O)) return fail("unit_columns", L, W, O, 0);
    printf("n=%d T=%d x=", n, p.T);
    for (int i = 0; i < n; i++) printf("%s%d", i ? "," : "", p.origin[(size_t)i]);
    printf(" w=");
    for (int i = 0; i < n; i++) printf("%s%d", i ? "," : "", p.width[(size_t)i]);
    printf(" c=");
    for (int i = 0; i < n; i++) printf("%s%d", i ? "," : "", p.bound[(size_t)i]);
    printf("\n");
  }
  return 0;
}
