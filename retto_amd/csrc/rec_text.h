// The rec tail's text front end: everything that turns text from outside the program into class ids -- the strict UTF-8
// decoder, the trimmed-line reader, the table of the dictionary's one-code-point classes, and on them the dictionary loader and
// the charset, lexicon and vocabulary compilers (the pattern compiler, ctc_pattern.h, reads its text with the same decoder and
// table).  Plain C++ as ctc_host_ref.h: no HIP, no session, so tests/native/rec_text_driver.cpp runs every byte index here under
// the sanitizers over exactly sized buffers.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/retto_hip.h"
#include "ctc_charset.h"
#include "ctc_lexicon.h"
#include "ctc_vocab.h"
#include "rt_error.h"

namespace rt {

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
inline int utf8_decode_strict(const unsigned char* p, size_t n, uint32_t* cp) {  // bytes consumed, 0 = invalid
  if (n == 0) return 0;
  const unsigned char c = p[0];
  if (c < 0x80) { *cp = c; return 1; }
  auto cont = [&](size_t i) { return i < n && (p[i] & 0xC0) == 0x80; };
  if (c >= 0xC2 && c <= 0xDF) { if (!cont(1)) return 0; *cp = ((c & 0x1Fu) << 6) | (p[1] & 0x3Fu); return 2; }
  if (c >= 0xE0 && c <= 0xEF) {
    if (!cont(1) || !cont(2)) return 0;
    if (c == 0xE0 && p[1] < 0xA0) return 0;   // overlong
    if (c == 0xED && p[1] >= 0xA0) return 0;  // surrogate
    *cp = ((c & 0x0Fu) << 12) | ((p[1] & 0x3Fu) << 6) | (p[2] & 0x3Fu); return 3;
  }
  if (c >= 0xF0 && c <= 0xF4) {
    if (!cont(1) || !cont(2) || !cont(3)) return 0;
    if (c == 0xF0 && p[1] < 0x90) return 0;   // overlong
    if (c == 0xF4 && p[1] >= 0x90) return 0;  // above U+10FFFF
    *cp = ((c & 0x07u) << 18) | ((p[1] & 0x3Fu) << 12) | ((p[2] & 0x3Fu) << 6) | (p[3] & 0x3Fu); return 4;
  }
  return 0;  // 0x80-0xC1 (continuation / overlong lead), 0xF5-0xFF
}
inline bool is_rust_whitespace(uint32_t c) {
  return (c >= 0x09 && c <= 0x0D) || c == 0x20 || c == 0x85 || c == 0xA0 || c == 0x1680 || (c >= 0x2000 && c <= 0x200A) ||
         c == 0x2028 || c == 0x2029 || c == 0x202F || c == 0x205F || c == 0x3000;
}

// The lines of text [len] as str::lines and str::trim give them: line(first, last_end) per line with the bytes of its trimmed
// text, first = NO_TEXT where nothing is left.  Every byte of a line is validated before its call.  Returns NO_TEXT, or the
// byte offset (from text) of the first malformed sequence, whose line and the ones behind it are not handed out.
constexpr size_t NO_TEXT = std::string::npos;
template <class F>
size_t trimmed_lines(const char* text, size_t len, F&& line) {
  const unsigned char* p = (const unsigned char*)text;
  for (size_t pos = 0; pos < len;) {
    size_t e = pos;   // one line: [pos, e) without its terminator
    while (e < len && p[e] != '\n') e++;
    size_t le = e;
    if (e < len && le > pos && p[le - 1] == '\r') le--;
    size_t first = NO_TEXT, last_end = 0;   // first / last non-whitespace char
    for (size_t i = pos; i < le;) {
      uint32_t cp;
      const int k = utf8_decode_strict(p + i, le - i, &cp);
      if (k == 0) return i;
      if (!is_rust_whitespace(cp)) { if (first == NO_TEXT) first = i; last_end = i + (size_t)k; }
      i += (size_t)k;
    }
    line(first, last_end);
    pos = e + 1;
  }
  return NO_TEXT;
}
// the code points of validated text [first, last_end)
inline void decode_into(const char* text, size_t first, size_t last_end, std::vector<uint32_t>& cps) {
  cps.clear();
  for (size_t i = first; i < last_end;) {
    uint32_t cp;
    i += (size_t)utf8_decode_strict((const unsigned char*)text + i, last_end - i, &cp);
    cps.push_back(cp);
  }
}
[[noreturn]] inline void throw_utf8(const char* what, size_t at) {
  throw RtError(RT_ERR_UTF8, std::string(what) + " is not valid UTF-8 (byte offset " + std::to_string(at) + ")");
}

// (code point, class) of every dictionary class >= 1 whose whole entry is one code point, sorted (class 0 is the blank,
// whatever its placeholder text).  Strict UTF-8 is canonical: an entry decodes to a code point iff its bytes are that code
// point's.
struct CodePointTable {
  typedef std::pair<uint32_t, int32_t> Entry;
  std::vector<Entry> v;
  explicit CodePointTable(const std::vector<std::string>& dict) {
    for (size_t c = 1; c < dict.size(); c++) {
      uint32_t cp;
      if (!dict[c].empty() && (size_t)utf8_decode_strict((const unsigned char*)dict[c].data(), dict[c].size(), &cp) == dict[c].size())
        v.push_back({cp, (int32_t)c});
    }
    std::sort(v.begin(), v.end());
  }
  // the first entry whose code point is cp or above, up to end()
  const Entry* from(uint32_t cp) const { return v.data() + (std::lower_bound(v.begin(), v.end(), Entry(cp, 0)) - v.begin()); }
  const Entry* end() const { return v.data() + v.size(); }
  // the lowest class of cp, or 0 where it has none
  int32_t lowest(uint32_t cp) const { const Entry* e = from(cp); return e != end() && e->first == cp ? e->second : 0; }
  // f(class) for every class of cp, ascending; false where it has none
  template <class F>
  bool all(uint32_t cp, F&& f) const {
    const Entry* e = from(cp);
    if (e == end() || e->first != cp) return false;
    for (; e != end() && e->first == cp; ++e) f(e->second);
    return true;
  }
};

// RecCharacter::new, above
inline std::vector<std::string> load_dictionary(const std::vector<uint8_t>& bytes) {
  const char* text = (const char*)bytes.data();
  std::vector<std::string> dict;
  dict.push_back("blank");
  const size_t bad = trimmed_lines(text, bytes.size(), [&](size_t first, size_t last_end) {
    dict.push_back(first == NO_TEXT ? std::string() : std::string(text + first, last_end - first));
  });
  if (bad != NO_TEXT) throw_utf8("dictionary", bad);
  dict.push_back(" ");
  return dict;
}

// A rec charset (ctc_charset.h) as its mask of cs::mask_words(dict.size()) words: the blank, every dictionary class whose whole
// entry is one code point of utf8 [len] (duplicates all join; U+0020 is the appended " "), and ids [n_ids].  Throws RT_ERR_UTF8
// for malformed text, RT_ERR_INVALID for a code point that matches no entry ("U+XXXX") or an id outside [0, dict.size()).
inline std::vector<uint32_t> compile_charset(const std::vector<std::string>& dict, const char* utf8, size_t len, const int32_t* ids,
                                             int n_ids) {
  const int classes = (int)dict.size();
  const CodePointTable one(dict);
  std::vector<uint32_t> mask((size_t)cs::mask_words(classes), 0u);
  auto add = [&](int c) { mask[(size_t)c >> 5] |= 1u << (c & 31); };
  add(0);
  for (size_t i = 0; i < len;) {
    uint32_t cp;
    const int k = utf8_decode_strict((const unsigned char*)utf8 + i, len - i, &cp);
    if (k == 0) throw_utf8("charset: the text", i);
    if (!one.all(cp, add)) {
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

// A rec lexicon (ctc_lexicon.h) as flat class ids and one length per entry: the lines of utf8 [len] (split and trimmed as the
// dictionary's lines are; empty lines skipped), each code point the LOWEST class id whose whole dictionary entry is that code
// point (U+0020 is the appended " "), then n_id_entries entries of entry_lens[i] ids each, consecutive in ids.  Throws RT_ERR_UTF8
// for malformed text; RT_ERR_INVALID for a code point that matches no entry ("U+XXXX", naming the entry), an id outside
// [1, dict.size()), an empty id entry, an entry longer than lx::MAX_LEN, or no entry at all; RT_ERR_CAPACITY past lx::MAX_ENTRIES.
inline void compile_lexicon(const std::vector<std::string>& dict, const char* utf8, size_t len, const int32_t* ids,
                            const int32_t* entry_lens, int n_id_entries, std::vector<int32_t>& ids_out, std::vector<int32_t>& lens_out) {
  const int classes = (int)dict.size();
  ids_out.clear(); lens_out.clear();
  const CodePointTable one(dict);
  auto entry_done = [&](int n) {
    if (n > lx::MAX_LEN)
      throw RtError(RT_ERR_INVALID, "lexicon: entry " + std::to_string(lens_out.size()) + " has " + std::to_string(n) +
                                        " tokens, more than RT_LEXICON_MAX_LEN (" + std::to_string(lx::MAX_LEN) + ")");
    if ((int)lens_out.size() >= lx::MAX_ENTRIES)
      throw RtError(RT_ERR_CAPACITY, "lexicon: more than RT_LEXICON_MAX_ENTRIES (" + std::to_string(lx::MAX_ENTRIES) + ") entries");
    lens_out.push_back(n);
  };
  std::vector<uint32_t> cps;
  const size_t bad = trimmed_lines(utf8, len, [&](size_t first, size_t last_end) {
    if (first == NO_TEXT) return;
    decode_into(utf8, first, last_end, cps);
    for (uint32_t cp : cps) {
      const int32_t c = one.lowest(cp);
      if (!c) {
        char b[96];
        snprintf(b, sizeof b, "lexicon: U+%04X in entry %zu matches no dictionary entry", (unsigned)cp, lens_out.size());
        throw RtError(RT_ERR_INVALID, b);
      }
      ids_out.push_back(c);
    }
    entry_done((int)cps.size());
  });
  if (bad != NO_TEXT) throw_utf8("lexicon: the text", bad);
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

// A vocabulary's words (ctc_vocab.h) in their id form: the lines of utf8 [len], split, trimmed and mapped as compile_lexicon maps
// them -- with flags & vc::CASE_VARIANTS each followed by the word with its first ASCII letter upper-cased and the word with all
// of them upper-cased, a variant with a code point the dictionary lacks being left out and counted -- then n_id_words words of
// word_lens[i] ids each.  A word already there is not added again.  Throws RT_ERR_UTF8 for malformed text; RT_ERR_INVALID, naming
// the word, for a code point that matches no entry ("U+XXXX"), the blank or an id outside [1, dict.size()), an empty or over-long
// word, no word at all, unknown flag bits; RT_ERR_CAPACITY past vc::MAX_WORDS.  The second form also compiles it (vc::compile).
inline void compile_vocab(const std::vector<std::string>& dict, const char* utf8, size_t len, const int32_t* ids, const int32_t* word_lens,
                          int n_id_words, int flags, vc::Ids& out, int* variants_dropped) {
  const int classes = (int)dict.size();
  out = vc::Ids{};
  *variants_dropped = 0;
  if (flags & ~vc::CASE_VARIANTS) {
    char b[64];
    snprintf(b, sizeof b, "vocab: unknown flag bits 0x%x", (unsigned)(flags & ~vc::CASE_VARIANTS));
    throw RtError(RT_ERR_INVALID, b);
  }
  const CodePointTable one(dict);
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
      const int32_t c = one.lowest(cp);
      if (!c) { *missing = cp; return false; }
      w.push_back(c);
    }
    return true;
  };
  auto lower = [](uint32_t c) { return c >= 'a' && c <= 'z'; };
  std::vector<uint32_t> cps, var;
  std::vector<int32_t> w;
  size_t n_text_words = 0;
  const size_t bad = trimmed_lines(utf8, len, [&](size_t first, size_t last_end) {
    if (first == NO_TEXT) return;
    const size_t word = n_text_words++;   // (the line's number among the lines that hold a word, for the messages)
    const std::string text(utf8 + first, std::min<size_t>(last_end - first, 48));   // (the start of the word, for the messages)
    decode_into(utf8, first, last_end, cps);
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
    if (!(flags & vc::CASE_VARIANTS)) return;
    for (int form = 0; form < 2; form++) {   // the first ASCII letter upper-cased; all of them
      var = cps;
      bool changed = false;
      for (uint32_t& c : var)
        if (lower(c)) { c -= 'a' - 'A'; changed = true; if (form == 0) break; }
        else if (form == 0 && c >= 'A' && c <= 'Z') break;   // (its first letter is a capital already)
      if (!changed) continue;
      if (to_ids(var, w, &missing)) add(w); else (*variants_dropped)++;
    }
  });
  if (bad != NO_TEXT) throw_utf8("vocab: the text", bad);
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
inline vc::Vocab compile_vocab(const std::vector<std::string>& dict, const char* utf8, size_t len, const int32_t* ids,
                               const int32_t* word_lens, int n_id_words, int flags, vc::Ids& f) {
  int dropped = 0;
  compile_vocab(dict, utf8, len, ids, word_lens, n_id_words, flags, f, &dropped);
  vc::Vocab m; std::string msg;
  const int rc = vc::compile((int)dict.size(), f, m, msg);
  if (rc != vc::OK) throw RtError(rc, msg);
  m.variants_dropped = dropped;
  return m;
}

}  // namespace rt
