// What the CTC tail of one rec group works on (rt_session::rec_tail, rec_tail.cpp), decided on the host in one place: the charset
// row tables, the lexicon, pattern, keyword and beam lines with their rows and tables, and the questions whose answers order the launches.  The
// pipeline (rec_groups) and the debug hooks (rt_debug_ctc_*) both go through it.  Plain C++ as lc_plan.h: built and checked
// without a GPU (tests/test_rec_tail_plan_cpu.py).
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "ctc_beam.h"
#include "ctc_keyword.h"
#include "ctc_lexicon.h"
#include "ctc_pattern.h"
#include "rec_line_opts.h"

namespace rt {

// One more line of a kind (lx::Line, or pt::Line: the same layout under other member names) and its T rows from row r0 of the
// group, behind the kind's earlier ones: what a line pass of the tail (rec_tail.cpp) stages and chunks.
template <class Line>
void add_line(std::vector<Line>& lines, std::vector<int>& rows, int r0, int T, int id, int slot, long long out) {
  lines.push_back(Line{(int)rows.size(), T, id, slot, out});
  for (int t = 0; t < T; t++) rows.push_back(r0 + t);
}

struct RecTailPlan {
  long long rows = 0;              // the group's time steps; every row below counts from the group's first
  // rec charsets (ctc_charset.h): every row's set (0: none) and the rows of the restricted lines in line order; both empty
  // when no row of the group is restricted
  std::vector<int> row_set, crows;
  // rec lexicons (ctc_lexicon.h): the group's lexicon lines in line order (row0 = the sum of the earlier ones' T, lex = the
  // 0-based lexicon, slot = the line's index in the call, out = the sum of the earlier ones' lexicon sizes), their rows line after
  // line, the floats of the loglik table and the largest lx::waves_of over the lines' lexicons
  std::vector<lx::Line> lines; std::vector<int> lrows;
  long long table = 0; int max_waves = 0;
  bool has_lex() const { return !lines.empty(); }   // (a lexicon line without a time step counts)
  bool table_fits() const { return table <= lx::MAX_GROUP_TABLE; }
  // lexicon snap (ctc_lexicon_align.h): a lexicon line of THIS group has min_posterior > 0; its lexicons then run before the decode
  bool snap = false;
  // rec patterns (ctc_pattern.h): the group's pattern lines and rows likewise (pat = the 0-based pattern, bp = the sum of the
  // earlier ones' backpointer codes), the largest P and S over the lines' patterns, and the backpointer codes the group's scratch
  // buffer holds: pt::bp_codes() of every line whose codes do not fit the kernel's LDS (pt::BP_LDS)
  std::vector<pt::Line> plines; std::vector<int> prows;
  int max_P = 0, max_S = 0; long long bp_codes = 0;
  bool has_pat() const { return !plines.empty(); }
  // rec keywords (ctc_keyword.h): the group's keyword lines and rows likewise (lex = the 0-based list, out = the sum of the
  // earlier ones' list sizes), the entries of the score / span table and the largest lx::waves_of over the lines' lists
  std::vector<kw::Line> klines; std::vector<int> krows;
  long long ktable = 0; int kmax_waves = 0;
  bool has_kw() const { return !klines.empty(); }   // (a keyword line without a time step counts)
  bool ktable_fits() const { return ktable <= lx::MAX_GROUP_TABLE; }
  // rec beams (ctc_beam.h; a session option, so every line of the group or none): the lines and rows likewise (lex = the first of
  // the line's trie nodes, out = the first of its N T token slots) and the trie nodes of the group, the sum of bm::nodes_of(T, B)
  std::vector<bm::Line> blines; std::vector<int> brows;
  long long bnodes = 0;
  bool has_beam() const { return !blines.empty(); }   // (a line without a time step counts: it reports 0 hypotheses)
  bool bnodes_fit() const { return bnodes <= bm::MAX_GROUP_NODES; }
  // the net must hand out the head's input: some logits are recomputed
  bool needs_z5(int cand_k) const { return cand_k > 1 || !crows.empty() || has_lex() || has_pat() || has_kw() || has_beam(); }
  // Why the group cannot run, or empty: its lexicon table, its keyword table or its trie (at beam width beam_b) is larger than a
  // group's may be.  rec_groups refuses such a group with RT_ERR_CAPACITY before its net runs.
  std::string refusal(int beam_b) const {
    if (!table_fits())
      return "rec lexicons: " + std::to_string(lines.size()) + " lines of one rec group carry lexicons of " + std::to_string(table) +
             " entries in all, more than the " + std::to_string(lx::MAX_GROUP_TABLE) +
             " likelihoods a group's table holds: use smaller lexicons or fewer lexicon lines per call";
    if (!ktable_fits())
      return "rec keywords: " + std::to_string(klines.size()) + " lines of one rec group carry keyword lists of " + std::to_string(ktable) +
             " entries in all, more than the " + std::to_string(lx::MAX_GROUP_TABLE) +
             " scores a group's table holds: use smaller keyword lists or fewer keyword lines per call";
    if (!bnodes_fit())
      return "rec beams: the " + std::to_string(blines.size()) + " lines of one rec group need " + std::to_string(bnodes) + " trie nodes at beam " +
             std::to_string(beam_b) + ", more than the " + std::to_string(bm::MAX_GROUP_NODES) + " a group's trie holds: use a narrower beam or fewer lines per call";
    return std::string();
  }
};

// The session's stores the plan reads (each null: no line has one): lexicon k is lex->lex[k - 1] and snaps where snap_min[k - 1] > 0
// (null: never); pattern k is pat->pats[k - 1]; keyword list k is kw->lex[k - 1]
struct RecStores { const lx::Tables* lex = nullptr; const float* snap_min = nullptr; const pt::Tables* pat = nullptr; const lx::Tables* kw = nullptr; };

// Lines [l0, l1) of a call: line li has the time steps [tok_off[li], tok_off[li + 1]) and the options line_opts[li] (rec_line_opts.h);
// beam_b > 0: the call's rec beam (rt_set_rec_beam: width and hypotheses per line)
inline RecTailPlan rec_tail_plan(const long long* tok_off, int l0, int l1, const RecLineOpts* line_opts, const RecStores& st,
                                 int beam_b = 0, int beam_n = 0) {
  RecTailPlan p;
  const long long t0 = tok_off[l0];
  p.rows = tok_off[l1] - t0;
  long long btok = 0;
  bool restricted = false;
  for (int li = l0; li < l1 && !restricted; li++) restricted = line_opts[li].charset > 0 && tok_off[li + 1] > tok_off[li];
  if (restricted) p.row_set.resize((size_t)p.rows);
  for (int li = l0; li < l1; li++) {
    const int r0 = (int)(tok_off[li] - t0), T = (int)(tok_off[li + 1] - tok_off[li]);
    const RecLineOpts& o = line_opts[li];
    for (int t = 0; restricted && t < T; t++) {
      p.row_set[(size_t)(r0 + t)] = o.charset;
      if (o.charset > 0) p.crows.push_back(r0 + t);
    }
    if (st.lex && o.lexicon > 0) {
      const lx::Lex& x = st.lex->lex[(size_t)o.lexicon - 1];
      add_line(p.lines, p.lrows, r0, T, o.lexicon - 1, li, p.table);
      p.table += x.n;
      p.max_waves = std::max(p.max_waves, lx::waves_of(x));
      p.snap = p.snap || (st.snap_min && st.snap_min[o.lexicon - 1] > 0.0f);
    }
    if (st.pat && o.pattern > 0) {
      const pt::Pat& a = st.pat->pats[(size_t)o.pattern - 1];
      add_line(p.plines, p.prows, r0, T, o.pattern - 1, li, p.bp_codes);
      p.max_P = std::max(p.max_P, a.P); p.max_S = std::max(p.max_S, a.S);
      if (pt::bp_codes(T, a.P, a.S) > pt::BP_LDS) p.bp_codes += pt::bp_codes(T, a.P, a.S);
    }
    if (st.kw && o.keywords > 0) {
      const lx::Lex& x = st.kw->lex[(size_t)o.keywords - 1];
      add_line(p.klines, p.krows, r0, T, o.keywords - 1, li, p.ktable);
      p.ktable += x.n;
      p.kmax_waves = std::max(p.kmax_waves, lx::waves_of(x));
    }
    if (beam_b > 0) {
      add_line(p.blines, p.brows, r0, T, (int)p.bnodes, li, btok);
      p.bnodes += bm::nodes_of(T, beam_b);
      btok += (long long)beam_n * T;
    }
  }
  return p;
}
// The same from one optional id array per kind (null: no line has one), as the plan tests' drivers hold them: lexicon k is
// tb.lex[k - 1], snap_min, ptb and ktb as RecStores'
inline RecTailPlan rec_tail_plan(const long long* tok_off, int l0, int l1, const int* line_set, const int* line_lex, const lx::Tables& tb,
                                 const float* snap_min, const int* line_pat = nullptr, const pt::Tables* ptb = nullptr,
                                 const int* line_kw = nullptr, const lx::Tables* ktb = nullptr, int beam_b = 0, int beam_n = 0) {
  std::vector<RecLineOpts> opts((size_t)l1);
  for (int li = l0; li < l1; li++)
    opts[(size_t)li] = {line_set ? line_set[li] : 0, line_lex ? line_lex[li] : 0, line_pat ? line_pat[li] : 0, line_kw ? line_kw[li] : 0};
  return rec_tail_plan(tok_off, l0, l1, opts.data(), RecStores{&tb, snap_min, ptb, ktb}, beam_b, beam_n);
}

}  // namespace rt
