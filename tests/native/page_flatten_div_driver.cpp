// Step 5 of the page flatten rule for every p in 0 .. 255 and L in 64 .. 16320 (tests/test_page_flatten_cpu.py): writes
// pf::flat_value as a [256][16257] byte table to argv[1]; prints how often pf::flat_value_rcp differs from it with the reciprocal
// rounded to nearest and one unit in the last place to either side (what v_rcp_f32 may return).
#include <cmath>
#include <cstdio>
#include <vector>
#include "page_flatten.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const int L0 = rt::pf::LEVEL_ONE, L1 = rt::pf::NUM;
  std::vector<unsigned char> table((size_t)256 * (L1 - L0 + 1));
  long differ = 0;
  for (int p = 0; p < 256; p++)
    for (int L = L0; L <= L1; L++) {
      const int v = rt::pf::flat_value(p, L);
      table[(size_t)p * (L1 - L0 + 1) + (L - L0)] = (unsigned char)v;
      const float rcp = 1.0f / (float)L;
      for (float x : {rcp, nextafterf(rcp, 0.0f), nextafterf(rcp, 1.0f)}) differ += rt::pf::flat_value_rcp(p, L, x) != v;
    }
  FILE* f = fopen(argv[1], "wb");
  if (!f || fwrite(table.data(), 1, table.size(), f) != table.size() || fclose(f)) return 1;
  printf("%ld\n", differ);
  return 0;
}
