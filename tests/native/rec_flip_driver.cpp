// Host-only driver for the rec flip rule (retto_amd/csrc/rec_flip.h), compiled with g++ -fsanitize=address,undefined by
// tests/test_rec_flip_cpu.py and run as a program: no GPU, nothing loaded into Python.  One query per input line:
//   c n0 bits0 n1 bits1     rf::choose of the two views' kept tokens and scores (floats as their 32 bits in hex, so NaN travels)
//   b scorebits belowbits   rf::check_param of cls_below, then both_ways / every_line / needs_scores
//   r n h1 w1 .. hn wn      the flat rotate index arithmetic over n crops, walked exactly as k_rec_flip_rotate walks it: byte i of
//                           the pool is (i * 7 + 3) mod 256; every destination pixel must be written once, from the pixel
//                           (h - 1 - y, w - 1 - x) of its own crop; answers the FNV-1a hash of the second region
// One answer line each.  The pool and the second region are heap blocks of exactly their sizes, so an index outside either ends
// the program under AddressSanitizer; a violated property ends it with status 2.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "rec_flip.h"

using namespace rt;

static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static int fail(const char* what, long long at) {
  fprintf(stderr, "rec_flip_driver: %s at %lld\n", what, at);
  return 2;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind;
    in >> kind;
    if (kind == "c") {
      int n0, n1; uint32_t b0, b1;
      in >> n0 >> std::hex >> b0 >> std::dec >> n1 >> std::hex >> b1;
      if (!in) { printf("bad query\n"); continue; }
      printf("%d\n", rf::choose(n0, from_bits(b0), n1, from_bits(b1)));
    } else if (kind == "b") {
      uint32_t bs, bb;
      in >> std::hex >> bs >> bb;
      if (!in) { printf("bad query\n"); continue; }
      const float sc = from_bits(bs), below = from_bits(bb);
      if (const char* why = rf::check_param(below)) { printf("invalid: %s\n", why); continue; }
      printf("both=%d every=%d needs=%d\n", rf::both_ways(sc, below) ? 1 : 0, rf::every_line(below) ? 1 : 0, rf::needs_scores(below) ? 1 : 0);
    } else if (kind == "r") {
      int n;
      in >> n;
      if (!in || n <= 0) { printf("bad query\n"); continue; }
      std::vector<int> hs((size_t)n), ws((size_t)n);
      std::vector<rf::FlipCrop> crops((size_t)n);
      long long pix = 0;
      for (int i = 0; i < n; i++) {
        in >> hs[(size_t)i] >> ws[(size_t)i];
        if (!in || hs[(size_t)i] <= 0 || ws[(size_t)i] <= 0) { n = -1; break; }
        const long long np = (long long)hs[(size_t)i] * ws[(size_t)i];
        crops[(size_t)i] = rf::FlipCrop{pix * 3, pix * 3, pix, np};   // (packed back to back on both sides, as rec_group_flip packs the second region)
        pix += np;
      }
      if (n < 0) { printf("bad query\n"); continue; }
      std::vector<uint8_t> pool((size_t)pix * 3), flipped((size_t)pix * 3, 0);
      std::vector<uint8_t> written((size_t)pix, 0);
      for (size_t i = 0; i < pool.size(); i++) pool[i] = (uint8_t)((i * 7 + 3) & 255);
      for (long long g = 0; g < pix; g++) {   // k_rec_flip_rotate's body for thread g
        const rf::FlipCrop& c = crops[(size_t)rf::find_crop(crops.data(), n, g)];
        const long long p = g - c.pix_base;
        if (p < 0 || p >= c.npix) return fail("pixel outside its crop", g);
        const uint8_t* a = pool.data() + c.src_off + rf::src_pixel(c.npix, p) * 3;
        uint8_t* q = flipped.data() + c.dst_off + p * 3;
        q[0] = a[0]; q[1] = a[1]; q[2] = a[2];
        if (written[(size_t)(c.dst_off / 3 + p)]++) return fail("pixel written twice", g);
      }
      for (int i = 0; i < n; i++)   // the definition: (y, x) <- (h - 1 - y, w - 1 - x), inside crop i
        for (int y = 0; y < hs[(size_t)i]; y++)
          for (int x = 0; x < ws[(size_t)i]; x++) {
            const long long d = crops[(size_t)i].dst_off + ((long long)y * ws[(size_t)i] + x) * 3;
            const long long s = crops[(size_t)i].src_off + ((long long)(hs[(size_t)i] - 1 - y) * ws[(size_t)i] + (ws[(size_t)i] - 1 - x)) * 3;
            if (!written[(size_t)(d / 3)]) return fail("pixel not written", d / 3);
            if (memcmp(&flipped[(size_t)d], &pool[(size_t)s], 3) != 0) return fail("pixel from the wrong place", d / 3);
          }
      unsigned long long h = 0xcbf29ce484222325ull;
      for (uint8_t b : flipped) h = (h ^ b) * 0x100000001b3ull;
      printf("%016llx\n", h);
    } else {
      printf("bad query\n");
    }
  }
  return 0;
}
