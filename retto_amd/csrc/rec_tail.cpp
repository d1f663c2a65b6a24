// The rec network's CTC tail and what feeds it: the dictionary, charset and lexicon text compilers, the session's charset and
// lexicon stores, the pattern pass (ctc_pattern.h), and rt_lane::rec_tail -- the one launch sequence behind the net that the
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
void compile_vocab(const std::vector<std::string>& dict, const char* utf8, size_t len, const int32_t* ids, const int32_t* word_lens,
                   int n_id_words, int flags, vc::Ids& out, int* variants_dropped) {
  const int classes = (int)dict.size();
  out = vc::Ids{};
  *variants_dropped = 0;
  if (flags & ~vc::CASE_VARIANTS) {
    char b[64];
    snprintf(b, sizeof b, "vocab: unknown flag bits 0x%x", (unsigned)(flags & ~vc::CASE_VARIANTS));
    throw RtError(RT_ERR_INVALID, b);
  }
  // every class whose whole entry is one code point, under its code point: the lowest id wins (as compile_lexicon)
  std::unordered_map<uint32_t, int> one;
  for (int c = classes - 1; c >= 1; c--) {
    const std::string& d = dict[(size_t)c];
    uint32_t cp;
    if (!d.empty() && (size_t)utf8_decode_strict((const unsigned char*)d.data(), d.size(), &cp) == d.size()) one[cp] = c;
  }
  std::unordered_map<std::string, int> seen;   // a word given twice is one word: the id form holds its first occurrence
  auto add = [&](const std::vector<int32_t>& w) {
    if (!seen.emplace(std::string((const char*)w.data(), w.size() * sizeof(int32_t)), 0).second) return;
    if (out.n() >= vc::MAX_WORDS)
      throw RtError(RT_ERR_CAPACITY, "vocab: more than RT_VOCAB_MAX_WORDS (" + std::to_string(vc::MAX_WORDS) + ") words");
    out.ids.insert(out.ids.end(), w.begin(), w.end()); out.lens.push_back((int32_t)w.size());
  };
  // the code points -> ids; false (nothing appended) where the dictionary lacks one, *missing = that code point
  auto to_ids = [&](const std::vector<uint32_t>& cps, std::vector<int32_t>& w, uint32_t* missing) {
    w.clear();
    for (uint32_t cp : cps) {
      const auto it = one.find(cp);
      if (it == one.end()) { *missing = cp; return false; }
      w.push_back(it->second);
    }
    return true;
  };
  auto lower = [](uint32_t c) { return c >= 'a' && c <= 'z'; };
  const unsigned char* p = (const unsigned char*)utf8;
  std::vector<uint32_t> cps, var;
  std::vector<int32_t> w;
  size_t word = 0;   // (the line's number among the lines that hold a word, for the messages)
  for (size_t pos = 0; pos < len; word++) {
    size_t e = pos;
    while (e < len && p[e] != '\n') e++;
    size_t le = e;
    if (e < len && le > pos && p[le - 1] == '\r') le--;
    size_t first = std::string::npos, last_end = 0;   // (trimmed as a dictionary line is)
    for (size_t i = pos; i < le;) {
      uint32_t cp;
      const int k = utf8_decode_strict(p + i, le - i, &cp);
      if (k == 0) throw RtError(RT_ERR_UTF8, "vocab: the text is not valid UTF-8 (byte offset " + std::to_string(i) + ")");
      if (!is_rust_whitespace(cp)) { if (first == std::string::npos) first = i; last_end = i + (size_t)k; }
      i += (size_t)k;
    }
    pos = e + 1;
    if (first == std::string::npos) { word--; continue; }
    const std::string text((const char*)p + first, std::min<size_t>(last_end - first, 48));   // (the start of the word, for the messages)
    cps.clear();
    for (size_t i = first; i < last_end;) {
      uint32_t cp;
      i += (size_t)utf8_decode_strict(p + i, last_end - i, &cp);
      cps.push_back(cp);
    }
    if ((int)cps.size() > vc::MAX_LEN)
      throw RtError(RT_ERR_INVALID, "vocab: word " + std::to_string(word) + " (\"" + text + "...\") has " + std::to_string(cps.size()) +
                                        " code points, more than RT_VOCAB_MAX_LEN (" + std::to_string(vc::MAX_LEN) + ")");
    uint32_t missing = 0;
    if (!to_ids(cps, w, &missing)) {
      char b[160];
      snprintf(b, sizeof b, "vocab: U+%04X in word %zu (\"%s\") matches no dictionary entry", (unsigned)missing, word, text.c_str());
      throw RtError(RT_ERR_INVALID, b);
    }
    add(w);
    if (!(flags & vc::CASE_VARIANTS)) continue;
    for (int form = 0; form < 2; form++) {   // the first ASCII letter upper-cased; all of them
      var = cps;
      bool changed = false;
      for (uint32_t& c : var)
        if (lower(c)) { c -= 'a' - 'A'; changed = true; if (form == 0) break; }
        else if (form == 0 && c >= 'A' && c <= 'Z') break;   // (its first letter is a capital already)
      if (!changed) continue;
      if (to_ids(var, w, &missing)) add(w); else (*variants_dropped)++;
    }
  }
  size_t o = 0;
  for (int j = 0; j < n_id_words; j++) {
    const int n = word_lens[j];
    if (n <= 0) throw RtError(RT_ERR_INVALID, "vocab: id word " + std::to_string(j) + " is empty");
    if (n > vc::MAX_LEN)
      throw RtError(RT_ERR_INVALID, "vocab: id word " + std::to_string(j) + " has " + std::to_string(n) + " ids, more than RT_VOCAB_MAX_LEN (" +
                                        std::to_string(vc::MAX_LEN) + ")");
    w.assign(ids + o, ids + o + (size_t)n);
    for (int c : w) {
      if (c == 0) throw RtError(RT_ERR_INVALID, "vocab: id word " + std::to_string(j) + ": the blank (class 0) is not a token");
      if (c < 0 || c >= classes)
        throw RtError(RT_ERR_INVALID, "vocab: class id " + std::to_string(c) + " in id word " + std::to_string(j) + " is outside [1, " +
                                          std::to_string(classes) + ")");
    }
    add(w);
    o += (size_t)n;
  }
  if (out.lens.empty()) throw RtError(RT_ERR_INVALID, "vocab: no word at all");
}
vc::Vocab compile_vocab(const std::vector<std::string>& dict, const char* utf8, size_t len, const int32_t* ids, const int32_t* word_lens,
                        int n_id_words, int flags, vc::Ids& f) {
  int dropped = 0;
  compile_vocab(dict, utf8, len, ids, word_lens, n_id_words, flags, f, &dropped);
  vc::Vocab m; std::string msg;
  const int rc = vc::compile((int)dict.size(), f, m, msg);
  if (rc != vc::OK) throw RtError(rc, msg);
  m.variants_dropped = dropped;
  return m;
}
}  // namespace rt

// ---- the tail of one rec group (session.h "the rec network's CTC tail") ----
namespace {
// a table of the plan through pinned staging into the scratch arena (an empty one gets one element and no copy)
template <typename T>
T* staged(rt_lane& s, const std::vector<T>& v) {
  const size_t n = std::max<size_t>(v.size(), 1);
  T* h = s.pinned.alloc<T>(n); T* d = s.scratch.alloc<T>(n);
  if (v.empty()) return d;
  memcpy(h, v.data(), v.size() * sizeof(T));
  RT_HIP_CHECK(hipMemcpyAsync(d, h, v.size() * sizeof(T), hipMemcpyHostToDevice, s.st));
  return d;
}
int chunk_rows_of(const rt_lane::RecTail& t) { return t.chunk_rows > 0 ? t.chunk_rows : cc::CAND_CHUNK; }
// The logits recompute every kind shares: up to `cap` rows of z5 gathered into zc, then the CTC FC -> logits [cap][ld].  Stream
// order lets a consumer's chunks share the two buffers.
struct LogitsChunk {
  rt_lane& s; const SvtrCore& core; const float* z5; int ld; float *zc, *logits;
  LogitsChunk(rt_lane& s_, const SvtrCore& core_, const float* z5_, int cap) : s(s_), core(core_), z5(z5_), ld(round_up(core_.classes, 4)) {
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
// Chunks of whole lines, so that a line's T rows are resident together: a chunk takes lines while their rows fit `chunk` and they
// are at most lx::LINES_PER_CHUNK, and always its first line.  Lines [i0, i1), whose rows are [r0, r0 + m) of the kind's row list;
// cap: raised to the largest m.
struct Chunk { int i0, i1, r0, m; };
template <typename Line>
std::vector<Chunk> line_chunks(const std::vector<Line>& lines, int chunk, int& cap) {
  std::vector<Chunk> out;
  const int n = (int)lines.size();
  for (int i0 = 0, i1; i0 < n; i0 = i1) {
    int rows = lines[i0].T;
    for (i1 = i0 + 1; i1 < n && i1 - i0 < lx::LINES_PER_CHUNK && rows + lines[i1].T <= chunk; i1++) rows += lines[i1].T;
    const int r0 = lines[i0].row0;
    out.push_back(Chunk{i0, i1, r0, lines[i1 - 1].row0 + lines[i1 - 1].T - r0});
    cap = std::max(cap, out.back().m);
  }
  return out;
}
// One pass over a kind's lines (session.h, above rec_tail): both tables staged, the logits and the row statistics the kind asks
// for (`stats`) sized by the largest chunk, `cap` rows, and shared by the chunks.  run(f): per chunk the row gather, the CTC FC,
// k_ctc_row_lse and k_ctc_row_max as asked, then f(the chunk's lines on the device, their number, r0, m) for the kind's own launches.
enum { ROW_LSE = 1, ROW_MAX = 2 };
template <typename Line>
struct LinePass {
  rt_lane& s;
  const Line* d_lines; const int* d_rows;
  int cap; std::vector<Chunk> chunks;
  LogitsChunk lc; float *lse, *rmax;
  LinePass(rt_lane& s_, const SvtrCore& core, const rt_lane::RecTail& t, const std::vector<Line>& lines, const std::vector<int>& rows, int stats)
      : s(s_), d_lines(staged(s_, lines)), d_rows(staged(s_, rows)), cap(1), chunks(line_chunks(lines, chunk_rows_of(t), cap)),
        lc(s_, core, t.z5, cap), lse(stats & ROW_LSE ? s_.scratch.alloc<float>((size_t)cap) : nullptr),
        rmax(stats & ROW_MAX ? s_.scratch.alloc<float>((size_t)cap) : nullptr) {}
  template <typename F>
  void run(F f) {
    for (const Chunk& c : chunks) {
      if (c.m > 0) {
        lc.run(d_rows + c.r0, c.m);
        if (lse) { ProfScope ps(&s.prof, s.st, "ctc_row_lse");
                   pp::ctc_row_lse(s.st, lc.logits, lc.ld, lc.core.classes, c.m, lse); }
        if (rmax) { ProfScope ps(&s.prof, s.st, "ctc_row_max");
                    pp::ctc_row_max(s.st, lc.logits, lc.ld, lc.core.classes, c.m, rmax); }
      }
      f(d_lines + c.i0, c.i1 - c.i0, c.r0, c.m);
    }
  }
};
// one table of a store (rt_entry_store, rt_patterns) into a device allocation of its own, with a blocking copy (an empty one gets
// one element and no copy); the store's holder frees it
template <typename T>
void upload_table(const T** d, const std::vector<T>& v) {
  RT_HIP_CHECK(hipMalloc((void**)d, std::max<size_t>(v.size(), 1) * sizeof(T)));
  if (!v.empty()) RT_HIP_CHECK(hipMemcpy(const_cast<T*>(*d), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
}
}  // namespace

void rt_lane::rec_tail(const RecTailPlan& p, const SvtrCore& core, const RecTail& t) {
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
    pp::word_boxes(st, t.idx, t.tok, t.ntok, t.wb->label, t.wb->cscore, sh->cfg.cls_thresh, t.wb->flip, sh->d_word_raw, dw, t.n_lines, t.wb->cols,
                   t.wb->n_words, t.wb->words);
  }
  if (!p.snap && p.has_lex()) ctc_lexicon(p, core, t);
  if (p.has_kw()) ctc_keywords(p, core, t);
  if (p.has_beam() && t.beam.b > 0) ctc_beams(p, core, t);
  if (t.cand.k > 0) ctc_candidates(core, t, p.rows, d_row_set);   // (before the caller rewinds the scratch arena z5 lives in)
}

void rt_lane::ctc_candidates(const SvtrCore& core, const RecTail& t, long long rows, const int* d_row_set) {
  const int K = t.cand.k;
  if (t.n_lines <= 0 || rows <= 0) return;
  int *kept_row = nullptr, *kept_slot = nullptr, *d_kept = nullptr;
  if (K > 1) { kept_row = scratch.alloc<int>((size_t)rows); kept_slot = scratch.alloc<int>((size_t)rows); d_kept = scratch.alloc<int>(1); }
  { ProfScope ps(&prof, st, "ctc_kept_rows");
    pp::ctc_kept_rows(st, t.idx, t.prob, t.lines, t.ntok, t.n_lines, K, t.cand.col, t.cand.cands, kept_row, kept_slot, d_kept); }
  if (K <= 1) return;
  // the only host wait of the option: the logits GEMMs are sized by the number of kept rows (about a tenth of the time steps)
  int* h_kept = pinned.alloc<int>(1);
  RT_HIP_CHECK(hipMemcpyAsync(h_kept, d_kept, sizeof(int), hipMemcpyDeviceToHost, st));
  sync();
  const int kept = (int)std::min<long long>(std::max(*h_kept, 0), rows);
  if (kept == 0) return;
  const int chunk = chunk_rows_of(t);
  LogitsChunk lc(*this, core, t.z5, std::min(chunk, kept));
  for (int c0 = 0; c0 < kept; c0 += chunk) {
    const int m = std::min(chunk, kept - c0);
    lc.run(kept_row + c0, m);
    ProfScope ps(&prof, st, "ctc_topk");
    pp::ctc_topk(st, lc.logits, lc.ld, core.classes, kept_slot + c0, m, K, t.cand.cands, kept_row + c0, d_row_set,
                 d_row_set ? t.charsets.masks : nullptr, t.charsets.words);
  }
}

void rt_lane::ctc_charset(const SvtrCore& core, const RecTail& t, const int* d_rows, int n_rows, const int* d_row_set) {
  if (n_rows <= 0) return;
  const int chunk = chunk_rows_of(t);
  LogitsChunk lc(*this, core, t.z5, std::min(chunk, n_rows));
  for (int c0 = 0; c0 < n_rows; c0 += chunk) {
    const int m = std::min(chunk, n_rows - c0);
    lc.run(d_rows + c0, m);
    ProfScope ps(&prof, st, "ctc_charset_argmax");
    pp::ctc_charset_argmax(st, lc.logits, lc.ld, core.classes, d_rows + c0, d_row_set, t.charsets.masks, t.charsets.words, m, t.idx, t.prob);
  }
}

void rt_lane::ctc_lexicon(const RecTailPlan& p, const SvtrCore& core, const RecTail& t) {
  const RecTail::Lexicon& o = t.lexicon;
  LinePass<lx::Line> pass(*this, core, t, p.lines, p.lrows, ROW_LSE);
  const LogitsChunk& lc = pass.lc;
  float* loglik = o.loglik ? o.loglik : scratch.alloc<float>((size_t)p.table);
  // (lexicon snap: the backpointers of a chunk's long lines, two 64-bit ballots per row)
  void* bp = p.snap ? scratch.alloc_bytes((size_t)pass.cap * 16) : nullptr;
  pass.run([&](const lx::Line* d_lines, int n, int r0, int) {
    { ProfScope ps(&prof, st, "ctc_lexicon_forward");
      pp::ctc_lexicon_forward(st, lc.logits, lc.ld, pass.lse, d_lines, n, r0, p.max_waves, o.d.lex, o.d.entries, o.d.order, o.d.ids, loglik); }
    if (p.snap) {   // (a line never straddles chunks: its matches are complete, and its logits still resident, here)
      { ProfScope ps(&prof, st, "ctc_lexicon_topk");
        pp::ctc_lexicon_topk(st, d_lines, n, o.d.lex, loglik, o.matches, o.n); }
      ProfScope ps(&prof, st, "ctc_lexicon_align");
      pp::ctc_lexicon_align(st, lc.logits, lc.ld, pass.lse, d_lines, n, r0, o.d.lex, o.d.entries, o.d.ids, o.d_min_post, o.matches, o.n,
                            pass.d_rows, bp, t.idx, t.prob, o.snapped, o.vit);
    }
  });
  if (!p.snap) {   // (without snap: one top-K over all the group's lines)
    ProfScope ps(&prof, st, "ctc_lexicon_topk");
    pp::ctc_lexicon_topk(st, pass.d_lines, (int)p.lines.size(), o.d.lex, loglik, o.matches, o.n);
  }
}

void rt_lane::ctc_pattern(const RecTailPlan& p, const SvtrCore& core, const RecTail& t) {
  const RecTail::Pattern& o = t.pattern;
  LinePass<pt::Line> pass(*this, core, t, p.plines, p.prows, ROW_LSE | ROW_MAX);
  const LogitsChunk& lc = pass.lc;
  // (the backpointer codes of the group's long lines, 16 bits each; every line has its own part: pt::Line::bp)
  void* bp = scratch.alloc_bytes((size_t)std::max<long long>(p.bp_codes, 1) * sizeof(uint16_t));
  pass.run([&](const pt::Line* d_lines, int n, int r0, int) {
    ProfScope ps(&prof, st, "ctc_pattern_viterbi");
    pp::ctc_pattern_viterbi(st, lc.logits, lc.ld, core.classes, pass.lse, pass.rmax, d_lines, n, r0, o.d, pass.d_rows, bp, t.idx, t.prob,
                            o.matched, o.vit, o.logprob, o.free_logprob);
  });
}

void rt_lane::ctc_keywords(const RecTailPlan& p, const SvtrCore& core, const RecTail& t) {
  const RecTail::Keywords& o = t.keywords;
  LinePass<kw::Line> pass(*this, core, t, p.klines, p.krows, ROW_MAX);
  const LogitsChunk& lc = pass.lc;
  const size_t table = (size_t)std::max<long long>(p.ktable, 1);
  float* score = o.score ? o.score : scratch.alloc<float>(table);
  int* span = o.span ? o.span : scratch.alloc<int>(2 * table);
  pass.run([&](const kw::Line* d_lines, int n, int r0, int) {
    ProfScope ps(&prof, st, "ctc_keyword_spot");
    pp::ctc_keyword_spot(st, lc.logits, lc.ld, pass.rmax, d_lines, n, r0, p.kmax_waves, o.d.lex, o.d.entries, o.d.order, o.d.ids, score, span);
  });
  ProfScope ps(&prof, st, "ctc_keyword_topk");
  pp::ctc_keyword_topk(st, pass.d_lines, (int)p.klines.size(), o.d.lex, o.d_min, score, span, o.hits, o.n);
}

void rt_lane::ctc_beams(const RecTailPlan& p, const SvtrCore& core, const RecTail& t) {
  const RecTail::Beam& o = t.beam;
  LinePass<bm::Line> pass(*this, core, t, p.blines, p.brows, ROW_LSE);
  const LogitsChunk& lc = pass.lc;
  bm::Node* nodes = scratch.alloc<bm::Node>((size_t)std::max<long long>(p.bnodes, 1));   // (the kernel initialises what it reads)
  bm::TopC* topc = scratch.alloc<bm::TopC>((size_t)pass.cap);   // (the chunks share it, as they share lse)
  pass.run([&](const bm::Line* d_lines, int n, int r0, int m) {
    if (m > 0) {
      ProfScope ps(&prof, st, "ctc_beam_topc");
      pp::ctc_beam_topc(st, lc.logits, lc.ld, core.classes, m, topc);
    }
    // (with a language model the search is its own profile family: its cost is then read off apart from the plain beam's)
    // (so is each instance with a word list)
    ProfScope ps(&prof, st, o.worded ? (o.fused ? "ctc_beam_search_lm_vocab" : "ctc_beam_search_vocab")
                                     : (o.fused ? "ctc_beam_search_lm" : "ctc_beam_search"));
    pp::ctc_beam_search(st, lc.logits, lc.ld, pass.lse, topc, d_lines, n, r0, o.b, o.n, nodes, o.recs, o.tok, o.count,
                        o.fused ? &o.fu : nullptr, o.lms, o.worded ? &o.wc : nullptr, o.vocs);
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

// ---- the entry stores (session.h rt_entry_store) ----
rt_entry_store::~rt_entry_store() {
  const void* p[] = {d.ids, d.entries, d.order, d.lex};
  for (const void* q : p) if (q) (void)hipFree(const_cast<void*>(q));
}
void rt_entry_store::set(lx::Tables fresh) {
  // the device tables are rebuilt whole (blocking copies; in a session no lane has work queued: the create calls are guarded and
  // every pipeline call ends with its streams drained)
  rt_entry_store up;   // (frees what it holds if a copy below throws; the old tables leave with it)
  upload_table(&up.d.ids, fresh.ids); upload_table(&up.d.entries, fresh.entries); upload_table(&up.d.order, fresh.order);
  upload_table(&up.d.lex, fresh.lex);
  std::swap(d, up.d);
  tb = std::move(fresh);
}
int rt_entry_store::add(const std::vector<std::string>& dict, const char* utf8, size_t len, const int32_t* ids, const int32_t* entry_lens,
                        int n) {
  std::unique_ptr<Host> h(new Host());
  compile_lexicon(dict, utf8, len, ids, entry_lens, n, h->ids, h->lens);
  int o = 0;
  for (int m : h->lens) {
    h->off.push_back(o);
    std::string t;
    for (int i = 0; i < m; i++) t += dict[(size_t)h->ids[(size_t)(o + i)]];
    h->text.push_back(std::move(t));
    o += m;
  }
  lx::Tables fresh = tb;
  fresh.add(h->ids.data(), h->lens.data(), (int)h->lens.size());
  host.reserve(host.size() + 1);   // (so that nothing behind set() throws)
  set(std::move(fresh));
  host.push_back(std::move(h));
  return (int)host.size();
}

int rt_session::lexicon_create(const char* utf8, size_t len, const int32_t* ids, const int32_t* entry_lens, int n_id_entries) {
  if ((int)lexicons->host.size() >= lx::MAX_LEXICONS)
    throw RtError(RT_ERR_CAPACITY, "rt_lexicon_create: the session holds RT_MAX_LEXICONS (" + std::to_string(lx::MAX_LEXICONS) + ") lexicons already");
  RT_HIP_CHECK(hipSetDevice(device));
  return lexicons->add(dict, utf8, len, ids, entry_lens, n_id_entries);
}

int rt_session::keywords_create(const char* utf8, size_t len, const int32_t* ids, const int32_t* entry_lens, int n_id_entries,
                                float min_score) {
  rt_keywords& X = *keywords;
  if (!(min_score <= 0.0f))   // (a NaN fails)
    throw RtError(RT_ERR_INVALID, "rt_keywords_create: min_score " + std::to_string(min_score) + " is not a number at most 0");
  if ((int)X.host.size() >= kw::MAX_LISTS)
    throw RtError(RT_ERR_CAPACITY, "rt_keywords_create: the session holds RT_MAX_KEYWORD_LISTS (" + std::to_string(kw::MAX_LISTS) + ") keyword lists already");
  std::vector<float> mins = X.min_score;
  mins.push_back(min_score);
  RT_HIP_CHECK(hipSetDevice(device));
  rt_keywords fresh;   // (holds the new min_score table until the entries are in, then leaves with the old one)
  upload_table(&fresh.d_min, mins);
  const int id = X.add(dict, utf8, len, ids, entry_lens, n_id_entries);
  std::swap(X.d_min, fresh.d_min);
  X.min_score = std::move(mins);
  return id;
}

// ---- the language models (session.h rt_lms) ----
namespace {
void free_view(const lm::View& v) {
  const void* p[] = {v.uni, v.states, v.arcs};
  for (const void* q : p) if (q) (void)hipFree(const_cast<void*>(q));
}
}  // namespace
rt_lms::~rt_lms() { for (const lm::View& v : dev) free_view(v); }
int rt_lms::add(lm::Model m) {
  host.reserve(host.size() + 1); dev.reserve(dev.size() + 1);   // (so that nothing behind the copies throws)
  std::unique_ptr<lm::Model> h(new lm::Model(std::move(m)));
  lm::View v = h->view();
  v.uni = nullptr; v.states = nullptr; v.arcs = nullptr;
  try {
    upload_table(&v.uni, h->uni); upload_table(&v.states, h->states); upload_table(&v.arcs, h->arcs);
  } catch (...) { free_view(v); throw; }
  host.push_back(std::move(h)); dev.push_back(v);
  return (int)host.size() - 1;
}
int rt_session::lm_create(const char* arpa, size_t len, float oov_log10) {
  if ((int)lms->host.size() >= lm::MAX_LMS)
    throw RtError(RT_ERR_CAPACITY, "rt_lm_create: the session holds RT_MAX_LMS (" + std::to_string(lm::MAX_LMS) + ") language models already");
  lm::Ids ids; lm::Model m; std::string msg;
  const int rc = lm::compile_arpa(dict, arpa, len, oov_log10, ids, m, msg);
  if (rc != lm::OK) throw RtError(rc, "rt_lm_create: " + msg);
  RT_HIP_CHECK(hipSetDevice(device));
  return lms->add(std::move(m));
}

// ---- the vocabularies (session.h rt_vocabs) ----
namespace {
void free_view(const vc::View& v) {
  const void* p[] = {v.nodes, v.arcs, v.mask, v.root};
  for (const void* q : p) if (q) (void)hipFree(const_cast<void*>(q));
}
}  // namespace
rt_vocabs::~rt_vocabs() { for (const vc::View& v : dev) free_view(v); }
int rt_vocabs::add(vc::Vocab m) {
  host.reserve(host.size() + 1); dev.reserve(dev.size() + 1);   // (so that nothing behind the copies throws)
  std::unique_ptr<vc::Vocab> h(new vc::Vocab(std::move(m)));
  vc::View v = h->view();
  v.nodes = nullptr; v.arcs = nullptr; v.mask = nullptr; v.root = nullptr;
  try {
    upload_table(&v.nodes, h->nodes); upload_table(&v.arcs, h->arcs); upload_table(&v.mask, h->mask); upload_table(&v.root, h->root);
  } catch (...) { free_view(v); throw; }
  host.push_back(std::move(h)); dev.push_back(v);
  return (int)host.size() - 1;
}
int rt_session::vocab_create(const char* utf8, size_t len, const int32_t* ids, const int32_t* word_lens, int n_id_words, int flags) {
  if ((int)vocabs->host.size() >= vc::MAX_VOCABS)
    throw RtError(RT_ERR_CAPACITY, "rt_vocab_create: the session holds RT_MAX_VOCABS (" + std::to_string(vc::MAX_VOCABS) + ") vocabularies already");
  vc::Ids f;
  vc::Vocab m;
  try { m = compile_vocab(dict, utf8, len, ids, word_lens, n_id_words, flags, f); }
  catch (const RtError& e) { throw RtError(e.code, std::string("rt_vocab_create: ") + e.what()); }
  RT_HIP_CHECK(hipSetDevice(device));
  return vocabs->add(std::move(m));
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
