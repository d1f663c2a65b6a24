// The rec network's CTC tail and what feeds it: the dictionary, charset and lexicon text compilers, the session's charset and
// lexicon stores, the pattern pass (ctc_pattern.h), and rt_session::rec_tail -- the one launch sequence behind the net that the
// pipeline (session.cpp rec_groups) and the debug hooks (api_debug.cpp rt_debug_ctc_*) both run, on the tables of rec_tail_plan.h.
#include "session.h"

#include <cstdio>
#include <cstring>
#include <unordered_map>

using namespace rt;

// ---------------------------------------------------------------------------
// RecCharacter::new (rec_processor.rs:29-46): String::from_utf8(bytes)? -> lines().map(|l| l.trim()) -> push " "
// -> insert "blank" at 0.  Rust semantics, restated exactly:
//  * String::from_utf8 is strict: overlong forms, surrogates (U+D800-DFFF) and code points above U+10FFFF
//    are errors (Utf8Error);
//  * str::lines splits after every '\n', drops that '\n' and one '\r' in front of it; a trailing '\n' does not
//    open a last empty line;
//  * str::trim strips every char with the Unicode White_Space property (char::is_whitespace): U+0009-000D,
//    U+0020, U+0085, U+00A0, U+1680, U+2000-200A, U+2028, U+2029, U+202F, U+205F, U+3000 -- a dictionary line
//    that holds only U+3000 becomes the empty string.
// ---------------------------------------------------------------------------
namespace rt {
static int utf8_decode_strict(const unsigned char* p, size_t n, uint32_t* cp) {  // bytes consumed, 0 = invalid
  if (n == 0) return 0;
  const unsigned char c = p[0];
  if (c < 0x80) { *cp = c; return 1; }
  auto cont = [&](size_t i) { return i < n && (p[i] & 0xC0) == 0x80; };
  if (c >= 0xC2 && c <= 0xDF) { if (!cont(1)) return 0; *cp = ((c & 0x1F) << 6) | (p[1] & 0x3F); return 2; }
  if (c >= 0xE0 && c <= 0xEF) {
    if (!cont(1) || !cont(2)) return 0;
    if (c == 0xE0 && p[1] < 0xA0) return 0;   // overlong
    if (c == 0xED && p[1] >= 0xA0) return 0;  // surrogate
    *cp = ((c & 0x0F) << 12) | ((p[1] & 0x3F) << 6) | (p[2] & 0x3F); return 3;
  }
  if (c >= 0xF0 && c <= 0xF4) {
    if (!cont(1) || !cont(2) || !cont(3)) return 0;
    if (c == 0xF0 && p[1] < 0x90) return 0;   // overlong
    if (c == 0xF4 && p[1] >= 0x90) return 0;  // above U+10FFFF
    *cp = ((c & 0x07) << 18) | ((p[1] & 0x3F) << 12) | ((p[2] & 0x3F) << 6) | (p[3] & 0x3F); return 4;
  }
  return 0;  // 0x80-0xC1 (continuation / overlong lead), 0xF5-0xFF
}
static bool is_rust_whitespace(uint32_t c) {
  return (c >= 0x09 && c <= 0x0D) || c == 0x20 || c == 0x85 || c == 0xA0 || c == 0x1680 || (c >= 0x2000 && c <= 0x200A) ||
         c == 0x2028 || c == 0x2029 || c == 0x202F || c == 0x205F || c == 0x3000;
}
std::vector<std::string> load_dictionary(const std::vector<uint8_t>& bytes) {
  const unsigned char* p = bytes.data();
  const size_t n = bytes.size();
  std::vector<std::string> dict;
  dict.push_back("blank");
  size_t pos = 0;
  while (pos < n) {
    // one line: [pos, e) without its terminator
    size_t e = pos;
    while (e < n && p[e] != '\n') e++;
    size_t le = e;
    if (e < n && le > pos && p[le - 1] == '\r') le--;
    // trim: first / last non-whitespace char, validating as we decode
    size_t first = std::string::npos, last_end = 0;
    for (size_t i = pos; i < le;) {
      uint32_t cp;
      int k = utf8_decode_strict(p + i, le - i, &cp);
      if (k == 0) throw RtError(RT_ERR_UTF8, "dictionary is not valid UTF-8 (byte offset " + std::to_string(i) + ")");
      if (!is_rust_whitespace(cp)) { if (first == std::string::npos) first = i; last_end = i + (size_t)k; }
      i += (size_t)k;
    }
    dict.push_back(first == std::string::npos ? std::string() : std::string((const char*)p + first, last_end - first));
    if (e >= n) break;
    pos = e + 1;
  }
  dict.push_back(" ");
  return dict;
}
std::vector<uint32_t> compile_charset(const std::vector<std::string>& dict, const char* utf8, size_t len, const int32_t* ids,
                                      int n_ids) {
  const int classes = (int)dict.size();
  std::vector<uint32_t> mask((size_t)cs::mask_words(classes), 0u);
  auto add = [&](int c) { mask[(size_t)c >> 5] |= 1u << (c & 31); };
  add(0);
  const unsigned char* p = (const unsigned char*)utf8;
  for (size_t i = 0; i < len;) {
    uint32_t cp;
    const int k = utf8_decode_strict(p + i, len - i, &cp);
    if (k == 0) throw RtError(RT_ERR_UTF8, "charset: the text is not valid UTF-8 (byte offset " + std::to_string(i) + ")");
    bool any = false;
    for (int c = 1; c < classes; c++)   // (class 0 is the blank, whatever its placeholder text)
      if (dict[(size_t)c].size() == (size_t)k && memcmp(dict[(size_t)c].data(), p + i, (size_t)k) == 0) { add(c); any = true; }
    if (!any) {
      char b[64];
      snprintf(b, sizeof b, "charset: U+%04X matches no dictionary entry", (unsigned)cp);
      throw RtError(RT_ERR_INVALID, b);
    }
    i += (size_t)k;
  }
  for (int j = 0; j < n_ids; j++) {
    if (ids[j] < 0 || ids[j] >= classes)
      throw RtError(RT_ERR_INVALID, "charset: class id " + std::to_string(ids[j]) + " is outside [0, " + std::to_string(classes) + ")");
    add(ids[j]);
  }
  return mask;
}
void compile_lexicon(const std::vector<std::string>& dict, const char* utf8, size_t len, const int32_t* ids,
                     const int32_t* entry_lens, int n_id_entries, std::vector<int32_t>& ids_out, std::vector<int32_t>& lens_out) {
  const int classes = (int)dict.size();
  ids_out.clear(); lens_out.clear();
  // every class whose whole entry is one code point, under its bytes: the lowest id wins (class 0 is the blank, whatever its
  // placeholder text)
  std::unordered_map<std::string, int> one;
  for (int c = classes - 1; c >= 1; c--) {
    const std::string& d = dict[(size_t)c];
    uint32_t cp;
    if (!d.empty() && (size_t)utf8_decode_strict((const unsigned char*)d.data(), d.size(), &cp) == d.size()) one[d] = c;
  }
  auto entry_done = [&](int n) {
    if (n > lx::MAX_LEN)
      throw RtError(RT_ERR_INVALID, "lexicon: entry " + std::to_string(lens_out.size()) + " has " + std::to_string(n) +
                                        " tokens, more than RT_LEXICON_MAX_LEN (" + std::to_string(lx::MAX_LEN) + ")");
    if ((int)lens_out.size() >= lx::MAX_ENTRIES)
      throw RtError(RT_ERR_CAPACITY, "lexicon: more than RT_LEXICON_MAX_ENTRIES (" + std::to_string(lx::MAX_ENTRIES) + ") entries");
    lens_out.push_back(n);
  };
  const unsigned char* p = (const unsigned char*)utf8;
  for (size_t pos = 0; pos < len;) {
    size_t e = pos;
    while (e < len && p[e] != '\n') e++;
    size_t le = e;
    if (e < len && le > pos && p[le - 1] == '\r') le--;
    size_t first = std::string::npos, last_end = 0;   // (trimmed as a dictionary line is)
    for (size_t i = pos; i < le;) {
      uint32_t cp;
      const int k = utf8_decode_strict(p + i, le - i, &cp);
      if (k == 0) throw RtError(RT_ERR_UTF8, "lexicon: the text is not valid UTF-8 (byte offset " + std::to_string(i) + ")");
      if (!is_rust_whitespace(cp)) { if (first == std::string::npos) first = i; last_end = i + (size_t)k; }
      i += (size_t)k;
    }
    if (first != std::string::npos) {
      int n = 0;
      for (size_t i = first; i < last_end;) {
        uint32_t cp;
        const int k = utf8_decode_strict(p + i, last_end - i, &cp);
        const auto it = one.find(std::string((const char*)p + i, (size_t)k));
        if (it == one.end()) {
          char b[96];
          snprintf(b, sizeof b, "lexicon: U+%04X in entry %zu matches no dictionary entry", (unsigned)cp, lens_out.size());
          throw RtError(RT_ERR_INVALID, b);
        }
        ids_out.push_back(it->second); n++;
        i += (size_t)k;
      }
      entry_done(n);
    }
    pos = e + 1;
  }
  size_t o = 0;
  for (int j = 0; j < n_id_entries; j++) {
    const int n = entry_lens[j];
    if (n <= 0) throw RtError(RT_ERR_INVALID, "lexicon: entry " + std::to_string(lens_out.size()) + " is empty");
    for (int i = 0; i < n && i < lx::MAX_LEN; i++) {
      const int c = ids[o + (size_t)i];
      if (c < 1 || c >= classes)
        throw RtError(RT_ERR_INVALID, "lexicon: class id " + std::to_string(c) + " in entry " + std::to_string(lens_out.size()) +
                                          " is outside [1, " + std::to_string(classes) + ")");
      ids_out.push_back(c);
    }
    entry_done(n);
    o += (size_t)n;
  }
  if (lens_out.empty()) throw RtError(RT_ERR_INVALID, "lexicon: no entry");
}
}  // namespace rt

// ---- the tail of one rec group (session.h "the rec network's CTC tail") ----
namespace {
// a table of the plan through pinned staging into the scratch arena (an empty one gets one element and no copy)
template <typename T>
T* staged(rt_session& s, const std::vector<T>& v) {
  const size_t n = std::max<size_t>(v.size(), 1);
  T* h = s.pinned.alloc<T>(n); T* d = s.scratch.alloc<T>(n);
  if (v.empty()) return d;
  memcpy(h, v.data(), v.size() * sizeof(T));
  RT_HIP_CHECK(hipMemcpyAsync(d, h, v.size() * sizeof(T), hipMemcpyHostToDevice, s.st));
  return d;
}
// The logits recompute the candidates, the charsets and the lexicons share: up to `cap` rows of z5 gathered into zc, then the
// CTC FC -> logits [cap][ld].  Stream order lets a consumer's chunks share the two buffers.
struct LogitsChunk {
  rt_session& s; const SvtrCore& core; const float* z5; int ld; float *zc, *logits;
  LogitsChunk(rt_session& s_, const SvtrCore& core_, const float* z5_, int cap) : s(s_), core(core_), z5(z5_), ld(round_up(core_.classes, 4)) {
    const size_t zc_n = ((size_t)cap + 256) * core.D;   // (zero rows past the chunk: a GEMM tile's loads stay inside the allocation)
    zc = s.scratch.alloc<float>(zc_n); logits = s.scratch.alloc<float>((size_t)cap * ld);
    RT_HIP_CHECK(hipMemsetAsync(zc, 0, zc_n * sizeof(float), s.st));
  }
  void run(const int* d_rows, int m) {   // rows d_rows[0..m) of z5 -> logits [m][ld]
    { ProfScope ps(&s.prof, s.st, "ctc_gather_rows");
      pp::ctc_gather_rows(s.st, z5, core.D, d_rows, m, zc); }
    RunCtx c = s.ctx(&s.scratch);
    core.logits_rows(c, zc, m, logits);
  }
};
// one table of a store (rt_lexicons, rt_patterns) into a device allocation of its own, with a blocking copy (an empty one gets one
// element and no copy); the store's holder frees it
template <typename T>
void upload_table(const T** d, const std::vector<T>& v) {
  RT_HIP_CHECK(hipMalloc((void**)d, std::max<size_t>(v.size(), 1) * sizeof(T)));
  if (!v.empty()) RT_HIP_CHECK(hipMemcpy(const_cast<T*>(*d), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
}
// Chunks of whole lines (lx::Line or pt::Line), so that a line's T rows are resident together: a chunk takes lines while their
// rows fit t.chunk_rows (0: cc::CAND_CHUNK) and they are at most lx::LINES_PER_CHUNK, and always its first line.  f(i0, i1, r0, m)
// per chunk: lines [i0, i1), whose rows are [r0, r0 + m) of the plan's compact row list.  Returns the largest m, at least 1.
template <typename Line, typename F>
int line_chunks(const std::vector<Line>& lines, const rt_session::RecTail& t, F f) {
  const int n = (int)lines.size(), chunk = t.chunk_rows > 0 ? t.chunk_rows : cc::CAND_CHUNK;
  int cap = 1;
  for (int i0 = 0, i1; i0 < n; i0 = i1) {
    int rows = lines[i0].T;
    for (i1 = i0 + 1; i1 < n && i1 - i0 < lx::LINES_PER_CHUNK && rows + lines[i1].T <= chunk; i1++) rows += lines[i1].T;
    const int r0 = lines[i0].row0, m = lines[i1 - 1].row0 + lines[i1 - 1].T - r0;
    f(i0, i1, r0, m);
    cap = std::max(cap, m);
  }
  return cap;
}
const auto no_chunk_work = [](int, int, int, int) {};   // (a pass of line_chunks for its result alone)
}  // namespace

void rt_session::rec_tail(const RecTailPlan& p, const SvtrCore& core, const RecTail& t) {
  const int* d_row_set = nullptr;
  if (!p.crows.empty()) {
    d_row_set = staged(*this, p.row_set);
    ctc_charset(core, t, staged(*this, p.crows), (int)p.crows.size(), d_row_set);
  }
  if (p.snap) ctc_lexicon(p, core, t);
  if (p.has_pat()) ctc_pattern(p, core, t);
  { ProfScope ps(&prof, st, "ctc_decode");
    pp::ctc_decode(st, t.idx, t.prob, t.lines, t.n_lines, t.tok, t.ntok, t.rscore); }
  if (t.wb) {
    pp::WordLineDesc* dw = scratch.alloc<pp::WordLineDesc>(t.n_lines);
    RT_HIP_CHECK(hipMemcpyAsync(dw, t.wb->h_lines, (size_t)t.n_lines * sizeof(pp::WordLineDesc), hipMemcpyHostToDevice, st));
    ProfScope ps(&prof, st, "word_boxes");
    pp::word_boxes(st, t.idx, t.tok, t.ntok, t.wb->label, t.wb->cscore, cfg.cls_thresh, d_word_raw, dw, t.n_lines, t.wb->cols,
                   t.wb->n_words, t.wb->words);
  }
  if (!p.snap) ctc_lexicon(p, core, t);
  if (p.has_kw()) ctc_keywords(p, core, t);
  if (p.has_beam()) ctc_beams(p, core, t);
  if (t.cand_k > 0) ctc_candidates(core, t, p.rows, d_row_set);   // (before the caller rewinds the scratch arena z5 lives in)
}

void rt_session::ctc_candidates(const SvtrCore& core, const RecTail& t, long long rows, const int* d_row_set) {
  const int K = t.cand_k;
  if (t.n_lines <= 0 || rows <= 0) return;
  int *kept_row = nullptr, *kept_slot = nullptr, *d_kept = nullptr;
  if (K > 1) { kept_row = scratch.alloc<int>((size_t)rows); kept_slot = scratch.alloc<int>((size_t)rows); d_kept = scratch.alloc<int>(1); }
  { ProfScope ps(&prof, st, "ctc_kept_rows");
    pp::ctc_kept_rows(st, t.idx, t.prob, t.lines, t.ntok, t.n_lines, K, t.ccol, t.cands, kept_row, kept_slot, d_kept); }
  if (K <= 1) return;
  // the only host wait of the option: the logits GEMMs are sized by the number of kept rows (about a tenth of the time steps)
  int* h_kept = pinned.alloc<int>(1);
  RT_HIP_CHECK(hipMemcpyAsync(h_kept, d_kept, sizeof(int), hipMemcpyDeviceToHost, st));
  sync();
  const int kept = (int)std::min<long long>(std::max(*h_kept, 0), rows);
  if (kept == 0) return;
  const int chunk = t.chunk_rows > 0 ? t.chunk_rows : cc::CAND_CHUNK;
  LogitsChunk lc(*this, core, t.z5, std::min(chunk, kept));
  for (int c0 = 0; c0 < kept; c0 += chunk) {
    const int m = std::min(chunk, kept - c0);
    lc.run(kept_row + c0, m);
    ProfScope ps(&prof, st, "ctc_topk");
    pp::ctc_topk(st, lc.logits, lc.ld, core.classes, kept_slot + c0, m, K, t.cands, kept_row + c0, d_row_set, d_row_set ? t.masks : nullptr, t.words);
  }
}

void rt_session::ctc_charset(const SvtrCore& core, const RecTail& t, const int* d_rows, int n_rows, const int* d_row_set) {
  if (n_rows <= 0) return;
  const int chunk = t.chunk_rows > 0 ? t.chunk_rows : cc::CAND_CHUNK;
  LogitsChunk lc(*this, core, t.z5, std::min(chunk, n_rows));
  for (int c0 = 0; c0 < n_rows; c0 += chunk) {
    const int m = std::min(chunk, n_rows - c0);
    lc.run(d_rows + c0, m);
    ProfScope ps(&prof, st, "ctc_charset_argmax");
    pp::ctc_charset_argmax(st, lc.logits, lc.ld, core.classes, d_rows + c0, d_row_set, t.masks, t.words, m, t.idx, t.prob);
  }
}

void rt_session::ctc_lexicon(const RecTailPlan& p, const SvtrCore& core, const RecTail& t) {
  const int n_lines = (int)p.lines.size();
  if (n_lines <= 0) return;
  const lx::Line* d_lines = staged(*this, p.lines); const int* d_rows = staged(*this, p.lrows);
  float* loglik = t.loglik ? t.loglik : scratch.alloc<float>((size_t)p.table);
  const lx::DevTables& X = t.d_lex;
  const int cap = line_chunks(p.lines, t, no_chunk_work);
  LogitsChunk lc(*this, core, t.z5, cap);
  float* lse = scratch.alloc<float>((size_t)cap);
  // (lexicon snap: the backpointers of a chunk's long lines, two 64-bit ballots per row)
  void* bp = p.snap ? scratch.alloc_bytes((size_t)cap * 16) : nullptr;
  line_chunks(p.lines, t, [&](int i0, int i1, int r0, int m) {   // (the chunks share lse too)
    if (m > 0) {
      lc.run(d_rows + r0, m);
      ProfScope ps(&prof, st, "ctc_row_lse");
      pp::ctc_row_lse(st, lc.logits, lc.ld, core.classes, m, lse);
    }
    { ProfScope ps(&prof, st, "ctc_lexicon_forward");
      pp::ctc_lexicon_forward(st, lc.logits, lc.ld, lse, d_lines + i0, i1 - i0, r0, p.max_waves, X.lex, X.entries, X.order, X.ids, loglik); }
    if (p.snap) {   // (a line never straddles chunks: its matches are complete, and its logits still resident, here)
      { ProfScope ps(&prof, st, "ctc_lexicon_topk");
        pp::ctc_lexicon_topk(st, d_lines + i0, i1 - i0, X.lex, loglik, t.lexm, t.lexn); }
      ProfScope ps(&prof, st, "ctc_lexicon_align");
      pp::ctc_lexicon_align(st, lc.logits, lc.ld, lse, d_lines + i0, i1 - i0, r0, X.lex, X.entries, X.ids, t.d_min_post, t.lexm, t.lexn,
                            d_rows, bp, t.idx, t.prob, t.lexs, t.vit);
    }
  });
  if (!p.snap) {   // (without snap: one top-K over all the group's lines)
    ProfScope ps(&prof, st, "ctc_lexicon_topk");
    pp::ctc_lexicon_topk(st, d_lines, n_lines, X.lex, loglik, t.lexm, t.lexn);
  }
}

void rt_session::ctc_pattern(const RecTailPlan& p, const SvtrCore& core, const RecTail& t) {
  if (p.plines.empty()) return;
  const pt::Line* d_lines = staged(*this, p.plines); const int* d_rows = staged(*this, p.prows);
  const int cap = line_chunks(p.plines, t, no_chunk_work);
  LogitsChunk lc(*this, core, t.z5, cap);
  float* lse = scratch.alloc<float>((size_t)cap); float* rmax = scratch.alloc<float>((size_t)cap);
  // (the backpointer codes of the group's long lines, 16 bits each; every line has its own part: pt::Line::bp)
  void* bp = scratch.alloc_bytes((size_t)std::max<long long>(p.bp_codes, 1) * sizeof(uint16_t));
  line_chunks(p.plines, t, [&](int i0, int i1, int r0, int m) {
    if (m > 0) {
      lc.run(d_rows + r0, m);
      { ProfScope ps(&prof, st, "ctc_row_lse");
        pp::ctc_row_lse(st, lc.logits, lc.ld, core.classes, m, lse); }
      ProfScope ps(&prof, st, "ctc_row_max");
      pp::ctc_row_max(st, lc.logits, lc.ld, core.classes, m, rmax);
    }
    ProfScope ps(&prof, st, "ctc_pattern_viterbi");
    pp::ctc_pattern_viterbi(st, lc.logits, lc.ld, core.classes, lse, rmax, d_lines + i0, i1 - i0, r0, t.d_pat, d_rows, bp, t.idx, t.prob,
                            t.patm, t.patv, t.patlp, t.patfree);
  });
}

void rt_session::ctc_keywords(const RecTailPlan& p, const SvtrCore& core, const RecTail& t) {
  const int n_lines = (int)p.klines.size();
  if (n_lines <= 0) return;
  const kw::Line* d_lines = staged(*this, p.klines); const int* d_rows = staged(*this, p.krows);
  const size_t table = (size_t)std::max<long long>(p.ktable, 1);
  float* score = t.kwscore ? t.kwscore : scratch.alloc<float>(table);
  int* span = t.kwspan ? t.kwspan : scratch.alloc<int>(2 * table);
  const lx::DevTables& X = t.d_kw;
  const int cap = line_chunks(p.klines, t, no_chunk_work);
  LogitsChunk lc(*this, core, t.z5, cap);
  float* rmax = scratch.alloc<float>((size_t)cap);
  line_chunks(p.klines, t, [&](int i0, int i1, int r0, int m) {   // (the chunks share rmax too)
    if (m > 0) {
      lc.run(d_rows + r0, m);
      ProfScope ps(&prof, st, "ctc_row_max");
      pp::ctc_row_max(st, lc.logits, lc.ld, core.classes, m, rmax);
    }
    ProfScope ps(&prof, st, "ctc_keyword_spot");
    pp::ctc_keyword_spot(st, lc.logits, lc.ld, rmax, d_lines + i0, i1 - i0, r0, p.kmax_waves, X.lex, X.entries, X.order, X.ids, score, span);
  });
  ProfScope ps(&prof, st, "ctc_keyword_topk");
  pp::ctc_keyword_topk(st, d_lines, n_lines, X.lex, t.d_kw_min, score, span, t.kwh, t.kwn);
}

void rt_session::ctc_beams(const RecTailPlan& p, const SvtrCore& core, const RecTail& t) {
  const int n_lines = (int)p.blines.size();
  if (n_lines <= 0 || t.beam_b <= 0) return;
  const bm::Line* d_lines = staged(*this, p.blines); const int* d_rows = staged(*this, p.brows);
  bm::Node* nodes = scratch.alloc<bm::Node>((size_t)std::max<long long>(p.bnodes, 1));   // (the kernel initialises what it reads)
  const int cap = line_chunks(p.blines, t, no_chunk_work);
  LogitsChunk lc(*this, core, t.z5, cap);
  float* lse = scratch.alloc<float>((size_t)cap); bm::TopC* topc = scratch.alloc<bm::TopC>((size_t)cap);
  line_chunks(p.blines, t, [&](int i0, int i1, int r0, int m) {   // (the chunks share lse and topc too)
    if (m > 0) {
      lc.run(d_rows + r0, m);
      { ProfScope ps(&prof, st, "ctc_row_lse");
        pp::ctc_row_lse(st, lc.logits, lc.ld, core.classes, m, lse); }
      ProfScope ps(&prof, st, "ctc_beam_topc");
      pp::ctc_beam_topc(st, lc.logits, lc.ld, core.classes, m, topc);
    }
    ProfScope ps(&prof, st, "ctc_beam_search");
    pp::ctc_beam_search(st, lc.logits, lc.ld, lse, topc, d_lines + i0, i1 - i0, r0, t.beam_b, t.beam_n, nodes, t.bmrec, t.bmtok, t.bmn);
  });
}

int rt_session::charset_create(const char* utf8, size_t len, const int32_t* ids, int n_ids) {
  rt_charsets& C = *charsets;
  if ((int)C.ids.size() >= cs::MAX_SETS)
    throw RtError(RT_ERR_CAPACITY, "rt_charset_create: the session holds RT_MAX_CHARSETS (" + std::to_string(cs::MAX_SETS) + ") charsets already");
  const std::vector<uint32_t> mask = compile_charset(dict, utf8, len, ids, n_ids);
  RT_HIP_CHECK(hipSetDevice(device));
  C.words = (int)mask.size();
  if (!C.d_masks) RT_HIP_CHECK(hipMalloc((void**)&C.d_masks, (size_t)cs::MAX_SETS * mask.size() * sizeof(uint32_t)));
  // (a blocking copy; no lane has work queued: this is a guarded call and every pipeline call ends with its streams drained)
  RT_HIP_CHECK(hipMemcpy(C.d_masks + C.ids.size() * mask.size(), mask.data(), mask.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  std::vector<int32_t> members;
  for (int c = 0; c < (int)dict.size(); c++) if (cs::allowed(mask.data(), c)) members.push_back(c);
  C.ids.push_back(std::move(members));
  return (int)C.ids.size();
}

int rt_session::lexicon_create(const char* utf8, size_t len, const int32_t* ids, const int32_t* entry_lens, int n_id_entries) {
  rt_lexicons& X = *lexicons;
  if ((int)X.host.size() >= lx::MAX_LEXICONS)
    throw RtError(RT_ERR_CAPACITY, "rt_lexicon_create: the session holds RT_MAX_LEXICONS (" + std::to_string(lx::MAX_LEXICONS) + ") lexicons already");
  std::unique_ptr<rt_lexicons::Host> h(new rt_lexicons::Host());
  compile_lexicon(dict, utf8, len, ids, entry_lens, n_id_entries, h->ids, h->lens);
  int o = 0;
  for (int n : h->lens) {
    h->off.push_back(o);
    std::string t;
    for (int i = 0; i < n; i++) t += dict[(size_t)h->ids[(size_t)(o + i)]];
    h->text.push_back(std::move(t));
    o += n;
  }
  lx::Tables tb = X.tb;
  tb.add(h->ids.data(), h->lens.data(), (int)h->lens.size());
  // the device tables are rebuilt whole (blocking copies; no lane has work queued: this is a guarded call and every pipeline
  // call ends with its streams drained)
  RT_HIP_CHECK(hipSetDevice(device));
  rt_lexicons fresh;   // (frees what it holds if a copy below throws)
  upload_table(&fresh.d.ids, tb.ids); upload_table(&fresh.d.entries, tb.entries); upload_table(&fresh.d.order, tb.order);
  upload_table(&fresh.d.lex, tb.lex);
  std::swap(X.d, fresh.d);   // (the old tables leave with `fresh`)
  X.tb = std::move(tb);
  X.host.push_back(std::move(h));
  return (int)X.host.size();
}

int rt_session::keywords_create(const char* utf8, size_t len, const int32_t* ids, const int32_t* entry_lens, int n_id_entries,
                                float min_score) {
  rt_keywords& X = *keywords;
  if (!(min_score <= 0.0f))   // (a NaN fails)
    throw RtError(RT_ERR_INVALID, "rt_keywords_create: min_score " + std::to_string(min_score) + " is not a number at most 0");
  if ((int)X.host.size() >= kw::MAX_LISTS)
    throw RtError(RT_ERR_CAPACITY, "rt_keywords_create: the session holds RT_MAX_KEYWORD_LISTS (" + std::to_string(kw::MAX_LISTS) + ") keyword lists already");
  std::unique_ptr<rt_lexicons::Host> h(new rt_lexicons::Host());
  compile_lexicon(dict, utf8, len, ids, entry_lens, n_id_entries, h->ids, h->lens);
  int o = 0;
  for (int n : h->lens) {
    h->off.push_back(o);
    std::string t;
    for (int i = 0; i < n; i++) t += dict[(size_t)h->ids[(size_t)(o + i)]];
    h->text.push_back(std::move(t));
    o += n;
  }
  lx::Tables tb = X.tb;
  tb.add(h->ids.data(), h->lens.data(), (int)h->lens.size());
  std::vector<float> mins = X.min_score;
  mins.push_back(min_score);
  // the device tables are rebuilt whole (blocking copies; no lane has work queued: this is a guarded call and every pipeline
  // call ends with its streams drained)
  RT_HIP_CHECK(hipSetDevice(device));
  rt_keywords fresh;   // (frees what it holds if a copy below throws)
  upload_table(&fresh.d.ids, tb.ids); upload_table(&fresh.d.entries, tb.entries); upload_table(&fresh.d.order, tb.order);
  upload_table(&fresh.d.lex, tb.lex); upload_table(&fresh.d_min, mins);
  std::swap(X.d, fresh.d); std::swap(X.d_min, fresh.d_min);   // (the old tables leave with `fresh`)
  X.tb = std::move(tb); X.min_score = std::move(mins);
  X.host.push_back(std::move(h));
  return (int)X.host.size();
}

int rt_session::pattern_create(const char* utf8, size_t len) {
  rt_patterns& X = *patterns;
  if ((int)X.host.size() >= pt::MAX_PATTERNS)
    throw RtError(RT_ERR_CAPACITY, "rt_pattern_create: the session holds RT_MAX_PATTERNS (" + std::to_string(pt::MAX_PATTERNS) + ") patterns already");
  pt::Compiled c;
  std::string msg;
  const int rc = pt::compile(dict, utf8, len, c, msg);
  if (rc != pt::OK) throw RtError(rc, msg);
  pt::Rule r;
  const std::string bad = r.build(c.classes, c.S, c.G, c.group_of.data(), c.delta.data(), c.accept.data());
  if (!bad.empty()) throw RtError(RT_ERR_INVALID, "pattern: " + bad);
  pt::Tables tb = X.tb;
  tb.add(r);
  // the device tables are rebuilt whole (blocking copies; no lane has work queued: this is a guarded call and every pipeline
  // call ends with its streams drained)
  RT_HIP_CHECK(hipSetDevice(device));
  rt_patterns fresh;   // (frees what it holds if a copy below throws)
  upload_table(&fresh.d.pats, tb.pats); upload_table(&fresh.d.pair_c, tb.pair_c); upload_table(&fresh.d.pair_pb, tb.pair_pb);
  upload_table(&fresh.d.pair_pe, tb.pair_pe); upload_table(&fresh.d.seg, tb.seg); upload_table(&fresh.d.preds, tb.preds);
  std::swap(X.d, fresh.d);   // (the old tables leave with `fresh`)
  X.tb = std::move(tb);
  X.host.emplace_back(new rt_patterns::Host{std::string(utf8, len), c.S, c.P, c.min_steps});
  return (int)X.host.size();
}

void rt_session::lexicon_set_snap(int lexicon, float min_posterior) {
  rt_lexicons& X = *lexicons;
  if (lexicon < 1 || lexicon > (int)X.host.size())
    throw RtError(RT_ERR_INVALID, "rt_lexicon_set_snap: unknown lexicon id " + std::to_string(lexicon));
  if (!(min_posterior >= 0.0f && min_posterior <= 1.0f))   // (a NaN fails both)
    throw RtError(RT_ERR_INVALID, "rt_lexicon_set_snap: min_posterior " + std::to_string(min_posterior) + " is outside [0, 1]");
  // (blocking copies; no lane has work queued: this is a guarded call and every pipeline call ends with its streams drained)
  RT_HIP_CHECK(hipSetDevice(device));
  if (!X.d_snap) {
    RT_HIP_CHECK(hipMalloc((void**)&X.d_snap, sizeof X.snap));
    RT_HIP_CHECK(hipMemcpy(X.d_snap, X.snap, sizeof X.snap, hipMemcpyHostToDevice));
  }
  RT_HIP_CHECK(hipMemcpy(X.d_snap + (lexicon - 1), &min_posterior, sizeof(float), hipMemcpyHostToDevice));
  X.snap[lexicon - 1] = min_posterior;
}
