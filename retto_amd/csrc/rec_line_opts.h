// The per-line options of the rec network's CTC tail -- a rec charset, a rec lexicon, a rec pattern, a rec keyword list -- as ONE
// value, and the host rules every road to the tail shares: which ids exist, "-1 means the session default", "a line may not carry
// both a pattern and a lexicon" (keywords only read a line: they go with anything), and how a call's regions or defaults become
// one entry per line.  A new option is a member of RecLineOpts and a row of REC_KINDS.  Plain C++ as rec_tail_plan.h and
// det_tiles.h: no HIP, no RtError (a function returns its message, empty = fine, and session.cpp / api.cpp wrap it in
// RT_ERR_INVALID); built and checked without a GPU (tests/test_rec_line_opts_cpu.py, tests/test_keyword_plan_cpu.py).
#pragma once
#include <algorithm>
#include <string>
#include <vector>

namespace rt {

// ids are 1-based (rt_charset_create / rt_lexicon_create / rt_pattern_create / rt_keywords_create), 0: none.  Also used as the
// number of ids of each kind a session holds (the largest valid id).
struct RecLineOpts { int charset = 0, lexicon = 0, pattern = 0, keywords = 0; };
// per kind: some line of the call has one
struct RecLineAny { bool charset = false, lexicon = false, pattern = false, keywords = false; };
// the kinds, in the order every check walks them; the first REC_WRITING_KINDS rewrite or rank the line and have rules among
// themselves, the keywords behind them only read it and are checked last
struct RecKind { const char* noun; int RecLineOpts::*id; bool RecLineAny::*any; };
constexpr int REC_N_KINDS = 4, REC_WRITING_KINDS = 3;
constexpr RecKind REC_KINDS[REC_N_KINDS] = {{"charset", &RecLineOpts::charset, &RecLineAny::charset},
                                            {"lexicon", &RecLineOpts::lexicon, &RecLineAny::lexicon},
                                            {"pattern", &RecLineOpts::pattern, &RecLineAny::pattern},
                                            {"keywords", &RecLineOpts::keywords, &RecLineAny::keywords}};

// n lines that carry ids[i] of one kind (null: none) and nothing else, as the rt_debug_ctc_* hooks' ABI and the plan tests'
// drivers hold them
inline std::vector<RecLineOpts> lines_with(int n, int RecLineOpts::*kind, const int* ids) {
  std::vector<RecLineOpts> lines((size_t)n);
  for (int i = 0; ids && i < n; i++) lines[(size_t)i].*kind = ids[i];
  return lines;
}

// The pattern's Viterbi and the lexicon's snap would both rewrite the line's rows, so a line carries at most one of the two.
inline bool carries_both(const RecLineOpts& o) { return o.pattern > 0 && o.lexicon > 0; }
// ... in words: `where` names a region ("page 0 region 2"), empty: o is the session's defaults
inline std::string rec_opts_conflict(const RecLineOpts& o, const std::string& where = std::string()) {
  if (!carries_both(o)) return std::string();
  return (where.empty() ? "the session defaults name both" : where + ": both") + " a rec pattern (" + std::to_string(o.pattern) +
         ") and a rec lexicon (" + std::to_string(o.lexicon) + "): a line may not carry both";
}

// rt_run_regions*, pages [p0, p1) of a call: region k of page i gets ids[j][i][k] of kind REC_KINDS[j], j < n_kinds (-1: the
// default `dflt`, 0: none, up to counts: that id; ids[j] or ids[j][i] null, or a kind past n_kinds: -1 throughout) -> out[i][k];
// out has an entry per page of the call.  Returns the first error in words ("page 1 region 2: unknown charset id 99"): pages in
// order, inside a page the charsets of all regions, then the lexicons, then the patterns, a region's conflict with its pattern,
// then the keywords.  (A range, so that run_regions can report a page's options behind the checks of its quads and before the
// next page's.)
inline std::string resolve_region_opts(int p0, int p1, const int* n_quads, const int* const* const* ids, int n_kinds,
                                       const RecLineOpts& dflt, const RecLineOpts& counts, std::vector<std::vector<RecLineOpts>>& out) {
  for (int i = p0; i < p1; i++) {
    out[(size_t)i].assign((size_t)n_quads[i], dflt);
    for (int j = 0; j < REC_N_KINDS; j++) {
      const RecKind& kind = REC_KINDS[j];
      for (int k = 0; k < n_quads[i]; k++) {
        RecLineOpts& o = out[(size_t)i][(size_t)k];
        const std::string where = "page " + std::to_string(i) + " region " + std::to_string(k);
        const int v = j < n_kinds && ids[j] && ids[j][i] ? ids[j][i][k] : -1;
        if (v < -1 || v > counts.*kind.id) return where + ": unknown " + kind.noun + " id " + std::to_string(v);
        if (v >= 0) o.*kind.id = v;
        if (j == 2 && carries_both(o)) return rec_opts_conflict(o, where);   // (every id of the region is resolved now)
      }
    }
  }
  return std::string();
}
// ... with the id arrays of the three writing kinds alone: every region takes the default keywords
inline std::string resolve_region_opts(int p0, int p1, const int* n_quads, const int* const* const ids[3], const RecLineOpts& dflt,
                                       const RecLineOpts& counts, std::vector<std::vector<RecLineOpts>>& out) {
  return resolve_region_opts(p0, p1, n_quads, ids, REC_WRITING_KINDS, dflt, counts, out);
}

// One entry per line of a call: line k of page i is line pages[i].first_line + k of the NL lines (the rec plan reorders widths,
// never lines) and gets page_opts[i][k], the regions' resolved options; page_opts null: every line gets `dflt`.  Page needs
// first_line and n_boxes.  any: per kind whether some line has one -- what decides whether the kind's buffers and results exist.
// Returns the first id of a writing kind outside [0, counts], the first line that carries both a pattern and a lexicon, or the
// first keywords id outside [0, counts], in words (the entry points refuse all three before anything is queued).
template <class Page>
std::string expand_line_opts(const Page* pages, int n_pages, int NL, const RecLineOpts* const* page_opts, const RecLineOpts& dflt,
                             const RecLineOpts& counts, std::vector<RecLineOpts>& lines, RecLineAny& any) {
  lines.assign((size_t)NL, page_opts ? RecLineOpts() : dflt);
  for (int i = 0; i < n_pages && page_opts; i++)
    std::copy(page_opts[i], page_opts[i] + pages[i].n_boxes, lines.begin() + pages[i].first_line);
  any = RecLineAny();
  for (int j = 0; j < REC_N_KINDS; j++) {
    const RecKind& kind = REC_KINDS[j];
    for (const RecLineOpts& o : lines) {
      const int v = o.*kind.id;
      if (v < 0 || v > counts.*kind.id) return std::string("unknown rec ") + kind.noun + " id " + std::to_string(v);
      any.*kind.any = any.*kind.any || v > 0;
    }
    if (j + 1 != REC_WRITING_KINDS) continue;   // (every writing kind of every line is known now)
    for (size_t li = 0; li < lines.size(); li++)
      if (carries_both(lines[li])) return "line " + std::to_string(li) + " carries both a rec pattern and a rec lexicon";
  }
  return std::string();
}

}  // namespace rt
