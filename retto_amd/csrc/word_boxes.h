// Word boxes from the rec CTC columns (rt_config.rec_return_word_box), written once for the device kernel (k_word_boxes,
// prepost_kernels.hip) and the CPU check (rt_debug_word_boxes).  The reference declares the option but never computes it
// (retto-core/src/processor/rec_processor.rs:48-56 `return_word_box // TODO`, its caller passes false at
// :199-206); the rule here is this project's own.  Its column-span model follows PaddleOCR's get_word_info /
// cal_ocr_word_box; unlike PaddleOCR the spans are mapped back through the crop's homography, so rotated det boxes and
// rotated crops come out right.  Translation units including this header are compiled with -ffp-contract=off: every f32
// expression rounds exactly as written, so host and device agree bit for bit.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "geom_math.h"

namespace rt {
namespace wb {

// raw class of a dictionary entry (one byte per class id, built once per session)
enum : uint8_t { RAW_SPLIT = 0, RAW_DIGIT = 1, RAW_ALPHA = 2, RAW_DOT = 3, RAW_HYPHEN = 4, RAW_CJK = 5 };
// effective class of a kept token
enum { EFF_SPLIT = 0, EFF_ALNUM = 1, EFF_CJK = 2 };
// word kind (rt_word.kind)
enum { KIND_CJK = 0, KIND_ALNUM = 1 };

// The line as the rec network saw it.  w_c x h_c: the crop after any rotate270; w x h, cw x ch: gm::crop_dims of the det box
// (pre-rotation); inv: the crop's output pixel -> page pixel homography (gm::projection_inverse).
struct WordGeom {
  int T, W, resized_w, w_c, h_c, rot270, w, h;
  float cw, ch;
  float inv[9];
};
// one word; the same layout as rt_word (include/retto_hip.h).  quad: TL, TR, BR, BL in after-resize_both page coordinates
// (the host applies gm::scale_and_clip).
struct Word {
  float quad[8];
  int32_t first_token, n_tokens, first_col, last_col, kind;
};

// Host only: the raw class of one UTF-8 dictionary entry.
inline uint8_t raw_class(const char* s, size_t len) {
  if (len == 0) return RAW_SPLIT;
  if (len == 1 && s[0] == '.') return RAW_DOT;
  if (len == 1 && s[0] == '-') return RAW_HYPHEN;
  bool digit = true, alnum = true;
  for (size_t i = 0; i < len; i++) {
    const unsigned char c = (unsigned char)s[i];
    const bool d = c >= '0' && c <= '9';
    const bool a = d || (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z');
    digit = digit && d; alnum = alnum && a;
  }
  if (digit) return RAW_DIGIT;
  if (alnum) return RAW_ALPHA;
  // every code point in U+4E00..U+9FFF: three-byte sequences E4 B8 80 .. E9 BF BF
  if (len % 3 != 0) return RAW_SPLIT;
  for (size_t i = 0; i < len; i += 3) {
    const unsigned char b0 = (unsigned char)s[i], b1 = (unsigned char)s[i + 1], b2 = (unsigned char)s[i + 2];
    if ((b0 & 0xF0) != 0xE0 || (b1 & 0xC0) != 0x80 || (b2 & 0xC0) != 0x80) return RAW_SPLIT;
    const uint32_t cp = ((uint32_t)(b0 & 0x0F) << 12) | ((uint32_t)(b1 & 0x3F) << 6) | (uint32_t)(b2 & 0x3F);
    if (cp < 0x4E00u || cp > 0x9FFFu) return RAW_SPLIT;
  }
  return RAW_CJK;
}

// effective class of token k from its raw class, the previous token's effective class and the next token's raw class
RT_HD int eff_class(int raw, int k, int n, int prev_eff, int next_raw) {
  switch (raw) {
    case RAW_DIGIT: case RAW_ALPHA: return EFF_ALNUM;
    case RAW_CJK: return EFF_CJK;
    case RAW_HYPHEN: return (k > 0 && prev_eff == EFF_ALNUM) ? EFF_ALNUM : EFF_SPLIT;
    case RAW_DOT: return (k > 0 && prev_eff == EFF_ALNUM && k + 1 < n && next_raw == RAW_DIGIT) ? EFF_ALNUM : EFF_SPLIT;
    default: return EFF_SPLIT;
  }
}

// rec-space span [x0, x1] of one word -> page quad (after resize_both coordinates)
RT_HD void span_to_quad(float x0, float x1, const WordGeom& g, int rot180, float* q) {
  const float wc = (float)g.w_c;
  x0 = fminf(fmaxf(x0, 0.0f), wc);
  x1 = fminf(fmaxf(x1, 0.0f), wc);
  if (rot180) { const float a = wc - x1, b = wc - x0; x0 = a; x1 = b; }
  float ua, ub, va, vb;
  if (!g.rot270) { ua = x0; ub = x1; va = 0.0f; vb = (float)g.h_c; }
  else { va = x0; vb = x1; ua = 0.0f; ub = (float)g.w; }   // k_warp_crops: out(col = y, row = w-1-x) = in(x, y)
  const float su = g.cw / (float)g.w, sv = g.ch / (float)g.h;
  const float Ua = ua * su, Ub = ub * su, Va = va * sv, Vb = vb * sv;
  const float U[4] = {Ua, Ub, Ub, Ua}, V[4] = {Va, Va, Vb, Vb};
  const float* i = g.inv;
  for (int c = 0; c < 4; c++) {
    const float dd = i[6] * U[c] + i[7] * V[c] + i[8];
    q[2 * c] = (i[0] * U[c] + i[1] * V[c] + i[2]) / dd;
    q[2 * c + 1] = (i[3] * U[c] + i[4] * V[c] + i[5]) / dd;
  }
}

// The words of one line.  ids[k] / cols[k]: class id and time step of kept token k (k < n, cols strictly increasing).
// raw_of_id: the session's class table.  Writes at most n words to out and returns their number.
RT_HD int line_words(const uint8_t* raw_of_id, const int* ids, const int* cols, int n, const WordGeom& g, int rot180,
                     Word* out) {
  if (n <= 0 || g.resized_w <= 0) return 0;
  const float p = ((float)g.W / (float)g.T) * ((float)g.w_c / (float)g.resized_w);   // crop pixels per column
  // pass 1: CJK pitch, the mean spacing over runs of >= 2 consecutive CJK tokens
  float dsum = 0.0f; int runs = 0;
  {
    int prev = EFF_SPLIT, run0 = -1;
    for (int k = 0; k <= n; k++) {
      int e = EFF_SPLIT;
      if (k < n) e = eff_class(raw_of_id[ids[k]], k, n, prev, k + 1 < n ? raw_of_id[ids[k + 1]] : RAW_SPLIT);
      if (e == EFF_CJK) { if (run0 < 0) run0 = k; }
      else if (run0 >= 0) {
        const int m = k - run0;
        if (m >= 2) { dsum = dsum + ((float)(cols[k - 1] - cols[run0]) * p) / (float)(m - 1); runs++; }
        run0 = -1;
      }
      prev = e;
    }
  }
  const float w_cjk = runs > 0 ? dsum / (float)runs : (float)g.w_c / (float)n;
  // pass 2: the words in token order
  int nw = 0, prev = EFF_SPLIT, a0 = -1;
  for (int k = 0; k <= n; k++) {
    int e = EFF_SPLIT;
    if (k < n) e = eff_class(raw_of_id[ids[k]], k, n, prev, k + 1 < n ? raw_of_id[ids[k + 1]] : RAW_SPLIT);
    if (e != EFF_ALNUM && a0 >= 0) {   // an ALNUM run a0 .. k-1 ends
      Word& w = out[nw++];
      span_to_quad((float)cols[a0] * p, (float)(cols[k - 1] + 1) * p, g, rot180, w.quad);
      w.first_token = a0; w.n_tokens = k - a0; w.first_col = cols[a0]; w.last_col = cols[k - 1]; w.kind = KIND_ALNUM;
      a0 = -1;
    }
    if (e == EFF_ALNUM && a0 < 0) a0 = k;
    if (e == EFF_CJK) {
      const float mid = ((float)cols[k] + 0.5f) * p;
      Word& w = out[nw++];
      span_to_quad(mid - 0.5f * w_cjk, mid + 0.5f * w_cjk, g, rot180, w.quad);
      w.first_token = k; w.n_tokens = 1; w.first_col = cols[k]; w.last_col = cols[k]; w.kind = KIND_CJK;
    }
    prev = e;
  }
  return nw;
}

}  // namespace wb
}  // namespace rt
