// Rows of an RGB8 page on the device, shared by page_enhance.hip and page_flatten.hip.  A page row is 3 w bytes, so most rows do
// not start on a dword.  A row segment of n pixels at byte address a is cut into items (row_item): the first a & 3 pixels (after
// k pixels the address is a + 3 k, a dword again at k = a & 3 mod 4), then groups of 4 pixels = 12 bytes = three dword accesses,
// then the rest.  Head and rest are moved as bytes.
#pragma once
#include <cstdint>

namespace rt {
namespace rows {

// Item j of a row segment of n pixels whose cut address is a: its first pixel and its number of pixels (0 .. 4); exactly 4 for
// the dword-aligned groups.  items_per_row(n) bounds the items of any such segment.
__device__ inline int items_per_row(int n) { return n / 4 + 2; }
__device__ inline int row_item(uintptr_t a, int n, int j, int* first) {
  const int head = min(n, (int)(a & 3)), groups = (n - head) >> 2;
  if (j == 0) { *first = 0; return head; }
  if (j <= groups) { *first = head + 4 * (j - 1); return 4; }
  *first = head + 4 * groups;
  return j == groups + 1 ? n - *first : 0;
}
// count (<= 4) pixels at p into px[k] = R | G << 8 | B << 16: three dword loads when there are 4 and p is a dword address
__device__ inline void load_pixels(const uint8_t* p, int count, uint32_t px[4]) {
  if (count == 4 && ((uintptr_t)p & 3) == 0) {
    const uint32_t* q = (const uint32_t*)p;
    const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
    px[0] = w0 & 0xffffffu;
    px[1] = (w0 >> 24) | ((w1 & 0xffffu) << 8);
    px[2] = (w1 >> 16) | ((w2 & 0xffu) << 16);
    px[3] = w2 >> 8;
  } else {
    for (int k = 0; k < 4; k++)
      px[k] = k < count ? (uint32_t)p[3 * k] | ((uint32_t)p[3 * k + 1] << 8) | ((uint32_t)p[3 * k + 2] << 16) : 0u;
  }
}
__device__ inline void store_pixels(uint8_t* p, int count, const uint32_t px[4]) {
  if (count == 4 && ((uintptr_t)p & 3) == 0) {
    uint32_t* q = (uint32_t*)p;
    q[0] = px[0] | (px[1] << 24);
    q[1] = (px[1] >> 8) | (px[2] << 16);
    q[2] = (px[2] >> 16) | (px[3] << 8);
  } else {
    for (int k = 0; k < count; k++) { p[3 * k] = (uint8_t)px[k]; p[3 * k + 1] = (uint8_t)(px[k] >> 8); p[3 * k + 2] = (uint8_t)(px[k] >> 16); }
  }
}

}  // namespace rows
}  // namespace rt
