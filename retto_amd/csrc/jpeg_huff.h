// JPEG entropy (Huffman) decoding shared by the gfx950 kernels (jpeg_huff.hip), the host preparation (image_decode.cpp) and the
// serial CPU check (rt_debug_jpeg_entropy, how = 2).  The method is self-synchronising parallel Huffman decoding (Weissenberger
// and Schmidt, "Massively Parallel Huffman Decoding on GPUs", ICPP 2018; applied to JPEG in their 2021 follow-up): the
// unstuffed entropy bytes of a page are cut into subsequences of HUFF_S bits, one lane decodes one subsequence from the guess
// "a block starts at my first bit", and lanes decode on into the following subsequences until their state agrees with the one
// stored there.  Every decode step is huff_decode_sub below, a restatement of JpegDec::decode_block in coefficient mode
// (image_decode.cpp) symbol for symbol, so the same bits give the same symbols on the host, in the kernels and in the check.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rt {
namespace jpeg {

// Subsequence length in bits.  Measured at 512 / 1024 / 2048 on 32 pages of 960 x 960: 512 is the fastest of the
// three -- a round of the synchronise pass costs one subsequence's serial decode, and the rounds dominate.
constexpr int HUFF_S = 512;
constexpr int HUFF_SUB_BYTES = HUFF_S / 8;
constexpr int HUFF_WG = 256;        // subsequences (lanes) per workgroup of the synchronise and write passes
constexpr int HUFF_MAX_WGS = 256;   // per page: the link pass gives every workgroup boundary of a page one lane of one workgroup
constexpr int HUFF_MAX_BPM = 10;    // blocks per MCU (T.81 B.2.3's limit for an interleaved scan)
constexpr int HUFF_PAD = 16;        // readable zero bytes behind a page's stream (a lane's 64-bit refill looks ahead)

// One Huffman table as the lanes look it up: JpegDec's Huff, field for field
struct HuffTab {
  uint16_t look[512];    // 9-bit lookahead: (length << 8) | symbol, 0 = longer code
  int32_t maxcode[18];
  int32_t valoff[17];
  uint8_t vals[256];
};
// The scan's geometry.  Scan-order block b is block b % bpm of MCU b / bpm; MCUs run in raster order, mcus_w per row; block k of
// an MCU belongs to component comp[k] and sits (bh[k], bv[k]) blocks into the MCU's hs x vs blocks of that component.
struct HuffGeom {
  int nc, bpm, mcus_w, total_mcus;
  int hs[3], vs[3], blocks_w[3];   // blocks_w: blocks per row of the MCU-padded plane
  uint8_t comp[HUFF_MAX_BPM], bh[HUFF_MAX_BPM], bv[HUFF_MAX_BPM];
  uint8_t pad_[2];
};
// One restart interval (the whole scan without restart markers).  It starts on a subsequence boundary of the page's stream.
struct HuffSeg {
  uint32_t first_sub;   // its first subsequence within the page
  uint32_t nbits;       // exact bit length
  uint32_t first_mcu, n_mcus;
};
// A lane's decoder state at a symbol boundary.  p: bit position inside the segment; kz: block within the MCU | zigzag index << 8
// (0 = the next symbol is a DC code); n: blocks completed inside the subsequence this state is the exit of.
struct HuffState {
  uint32_t p, kz, n;
};
constexpr uint32_t HUFF_INVALID = 0xffffffffu;   // p of a state nothing can follow (the guess met an impossible code)

__host__ __device__ inline uint32_t huff_seg_subs(const HuffSeg& sg) {
  const uint32_t k = (sg.nbits + HUFF_S - 1) / HUFF_S;
  return k ? k : 1;
}
__host__ __device__ inline int huff_zigzag(int k) {
  constexpr uint8_t z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return z[k];
}
__host__ __device__ inline int huff_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// Offset (in int16 units) of scan-order block b inside its component's coefficient plane, and that component
__host__ __device__ inline size_t huff_block_pos(const HuffGeom& G, uint32_t b, int* comp) {
  const uint32_t mcu = b / (uint32_t)G.bpm, k = b - mcu * (uint32_t)G.bpm;
  const uint32_t my = mcu / (uint32_t)G.mcus_w, mx = mcu - my * (uint32_t)G.mcus_w;
  const int c = G.comp[k];
  *comp = c;
  return ((size_t)(my * G.vs[c] + G.bv[k]) * G.blocks_w[c] + mx * G.hs[c] + G.bh[k]) * 64;
}
// The same for the i-th block of component c in scan order from MCU first_mcu on (the DC pass)
__host__ __device__ inline size_t huff_comp_block_pos(const HuffGeom& G, int c, uint32_t first_mcu, uint32_t i) {
  const uint32_t bc = (uint32_t)(G.hs[c] * G.vs[c]);
  const uint32_t mcu = first_mcu + i / bc, j = i % bc, v = j / (uint32_t)G.hs[c], h = j % (uint32_t)G.hs[c];
  const uint32_t my = mcu / (uint32_t)G.mcus_w, mx = mcu - my * (uint32_t)G.mcus_w;
  return ((size_t)(my * G.vs[c] + v) * G.blocks_w[c] + mx * G.hs[c] + h) * 64;
}

// A lane's view of the stream: bytes s[0, limit), 64-bit bit buffer, most significant bit first.  Bytes outside read as zero,
// so no position a damaged stream can produce reads out of bounds.
struct HuffReader {
  const uint8_t* s;
  int pos;
  uint32_t limit;
  uint64_t bits;
  int n;
  __host__ __device__ inline void fill() {
    while (n <= 56) {
      const uint64_t b = (uint32_t)pos < limit ? s[pos] : 0;
      pos++;
      bits |= b << (56 - n);
      n += 8;
    }
  }
  __host__ __device__ inline void seek(int seg_byte, uint32_t bit) {
    pos = seg_byte + (int)(bit >> 3); bits = 0; n = 0;
    fill();
    drop((int)(bit & 7));
  }
  __host__ __device__ inline void drop(int l) { bits <<= l; n -= l; }
};

// JpegDec::decode: the symbol at the head of `bits`; *len = its code length, 17 = no code of up to 16 bits matches
__host__ __device__ inline int huff_symbol(const HuffTab& h, uint64_t bits, int* len) {
  const uint16_t e = h.look[bits >> 55];
  if (e) { *len = e >> 8; return e & 0xff; }
  int code = (int)(bits >> 54), l = 10;
  for (; l <= 16; l++) {
    if (code <= h.maxcode[l]) break;
    code = (int)(bits >> (64 - l - 1));
  }
  *len = l;
  return l > 16 ? 0 : h.vals[(code + h.valoff[l]) & 0xff];
}

enum { HUFF_OK = 0, HUFF_END = 1, HUFF_BAD = 2 };

// Decodes the symbols that START in bits [st.p, end) of a segment (end <= seg_bits) from entry state st, which becomes the exit
// state.  s + seg_byte is the segment's first byte.  tabs: DC table of component c at 2 c, AC at 2 c + 1.  sink.block(n) gives
// where the n-th block touched by this call goes (null: nowhere), sink.put stores one coefficient; the DC value is stored as
// its difference.  Every iteration consumes at least one bit.  HUFF_END: the next symbol would read past the segment (st stays at
// its first bit); HUFF_BAD: what JpegDec rejects -- no code of up to 16 bits, a DC size above 11, a zigzag index above 63.
template <class Sink>
__host__ __device__ inline int huff_decode_sub(const HuffTab* tabs, const HuffGeom& G, const uint8_t* s, int seg_byte, uint32_t limit,
                                               uint32_t seg_bits, uint32_t end, HuffState& st, Sink& sink) {
  uint32_t p = st.p, n = 0;
  int k = (int)(st.kz & 0xff), z = (int)(st.kz >> 8), status = HUFF_OK;
  HuffReader rd{s, 0, limit, 0, 0};
  rd.seek(seg_byte, p);
  int16_t* blk = sink.block(0);
  while (p < end) {
    if (rd.n < 32) rd.fill();
    int l;
    const int sym = huff_symbol(tabs[2 * G.comp[k] + (z ? 1 : 0)], rd.bits, &l);
    const uint32_t left = seg_bits - p;
    if ((uint32_t)l > left) { status = (l > 16 && left >= 16) ? HUFF_BAD : HUFF_END; break; }
    if (l > 16 || (z == 0 && sym > 11)) { status = HUFF_BAD; break; }
    const int sz = z ? (sym & 15) : sym, run = z ? (sym >> 4) : 0;
    if ((uint32_t)(l + sz) > left) { status = HUFF_END; break; }
    rd.drop(l);
    int v = 0;
    if (sz) { v = huff_extend((int)(rd.bits >> (64 - sz)), sz); rd.drop(sz); }
    p += (uint32_t)(l + sz);
    bool done = false;
    if (z == 0) { if (v) sink.put(blk, 0, v); z = 1; }
    else if (sz == 0) { if (run != 15) done = true; else { z += 16; done = z > 63; } }
    else {
      z += run;
      if (z > 63) { status = HUFF_BAD; break; }
      sink.put(blk, huff_zigzag(z), v);
      z++;
      done = z > 63;
    }
    if (done) { z = 0; n++; k = k + 1 == G.bpm ? 0 : k + 1; blk = sink.block(n); }
  }
  st.p = p; st.kz = (uint32_t)k | ((uint32_t)z << 8); st.n = n;
  return status;
}

// The sink of the synchronisation passes: states only
struct HuffNoSink {
  __host__ __device__ inline int16_t* block(uint32_t) { return nullptr; }
  __host__ __device__ inline void put(int16_t*, int, int) {}
};
// The sink of the write pass: block first + n of the scan, as long as it lies inside the segment (a damaged stream may decode more
// blocks than the segment has; the count check flags it, nothing is written for them)
struct HuffCoefSink {
  const HuffGeom* G;
  int16_t* plane[3];
  uint32_t first, seg_end;
  __host__ __device__ inline int16_t* block(uint32_t n) {
    const uint32_t b = first + n;
    if (b >= seg_end) return nullptr;
    int c;
    const size_t at = huff_block_pos(*G, b, &c);
    return plane[c] + at;
  }
  __host__ __device__ inline void put(int16_t* blk, int at, int v) { if (blk) blk[at] = (int16_t)v; }
};

// What must hold where a segment's last subsequence ends: the predicted block count, a block boundary, fewer than 8 unread bits
__host__ __device__ inline bool huff_seg_end_ok(const HuffSeg& sg, const HuffGeom& G, const HuffState& exit, uint32_t blocks_before) {
  return blocks_before + exit.n == (sg.first_mcu + sg.n_mcus) * (uint32_t)G.bpm && (exit.kz >> 8) == 0 && sg.nbits - exit.p < 8;
}

// One page for the kernels.  Offsets are bytes from the slot's base.
struct DevHuffPage {
  uint64_t stream_off, tabs_off, segs_off;   // nsubs * HUFF_SUB_BYTES + HUFF_PAD bytes; HuffTab[6]; HuffSeg[nsegs]
  uint64_t state_off, first_off;             // HuffState[nsubs]; uint32_t[nsubs]: scan-order index of a subsequence's first block
  uint64_t coef_off[3];
  uint32_t coef_bytes[3];
  uint32_t nsubs, nsegs, nwg;
  uint32_t wg_base, seg_base;                // prefix sums over the launch's pages
  HuffGeom G;
};
// per page, behind the launch's DevHuffPage table: [0] flag, [1] rounds of the synchronise pass, [2] of the link pass
constexpr int HUFF_INFO = 3;

}  // namespace jpeg

// jpeg_huff.hip: passes 1-5 for every page of one lane part, on `st`.  pages / info: device addresses inside the slot `base`.
// hpages: the same table on the host (launch sizes).
void launch_jpeg_huff(uint8_t* base, const jpeg::DevHuffPage* pages, int* info, const jpeg::DevHuffPage* hpages, int npages,
                      hipStream_t st);

}  // namespace rt
