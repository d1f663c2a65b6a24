// Host-only driver of nn::gemm_plan() / nn::gemm_se_rows() (retto_amd/csrc/gemm_plan.cpp) and nn::dw_plan() / nn::lc_plan()
// (lc_plan.cpp) for tests/test_gemm_plan_cpu.py and tests/test_lc_plan_cpu.py, and of the host-only headers rec_tail_plan.h
// (tests/test_rec_tail_plan_cpu.py), rec_line_opts.h (tests/test_rec_line_opts_cpu.py) and lane_split.h (tests/test_lane_split_cpu.py).
// One query per stdin line, one answer per stdout line:
//   plan <variant> <dma> <split> <argmax_wide> <cus> <lda> <M> <K> <N> <Npad16> <ldc> <coff>
//        <am_max> <residual> <a_scale> <a_tab_stride> <act> <has_lab> <n_img> <ld_scale>
//     -> <kernel> <nt> <kg> <bf> <se> <grid_x> <grid_y> <label, or the error of an invalid plan>
//   se_rows <variant> <dma> <split> <lda> <M> <K> <N> <Npad16> <act> <min_pix>  ->  <rows>
//   dw <dw_sweep> <K> <sh> <sw> <Cp> <maxHo> <maxWo> <pooled>
//     -> <kernel> <sweep instance, or 0> <R> <lanes> <strips per block> <chunks> <grid_x> <grid_z>
//   lc <lc_wave> <dw_sweep> <K> <sh> <sw> <Cp> <C> <N> <Npad16> <dw_act> <dw_has_lab> <se> <maxHo> <maxWo> <rows> <min_pix>
//      <pw_act> <pw_has_lab> <pw_bias>          (the output pitch is chan_pitch(N), as run_lc's)
//     (lc_wave / dw_sweep -1: what the environment selected when the driver started)
//     -> thin | wave | lds <instance> <tile rows> <grid_x>    or    unfused <se_rows> <the block's dw answer>
//   tail <l0> <l1> <cand_k> <NL> <T of each of the NL lines> <1 + NL charset ids, or 0> <1 + NL lexicon ids, or 0>
//        <n_lex> <n16 n32 n64 of each lexicon: its entries of 1, 8 and 16 ids> <1 + n_lex snap thresholds, or 0>
//     -> rec_tail_plan() (rec_tail_plan.h) of lines [l0, l1): rows=.. z5=.. has_lex=.. snap=.. table=.. fits=.. max_waves=..
//        row_set=a,b,.. crows=.. lines=row0:T:lex:slot:out,.. lrows=..   (an empty list prints as -)
//   group <l0> <l1> <beam> <nbest> <NL> <T of each line> <n_lex> <n16 n32 n64 of each lexicon> <a snap threshold per lexicon>
//         <n_kw> <n16 n32 n64 of each keyword list> <n_pat> <S P of each pattern> <charset lexicon pattern keywords of each line>
//     -> rec_tail_plan() of lines [l0, l1) with every kind at once: row_set=.. crows=.. lines=.. lrows=.. plines=row0:T:pat:slot:bp,..
//        prows=.. klines=row0:T:list:slot:out,.. krows=.. blines=row0:T:node0:slot:out,.. brows=..
//   capacity <the arguments of group>  ->  RecTailPlan::refusal(beam) of that group, or -
//   defaults <charset> <lexicon> <pattern>  ->  rec_opts_conflict() of session defaults: ok   or   error: <message>
//   regions <default charset lexicon pattern> <count of charsets lexicons patterns> <n_pages> <regions of each page>
//           then per kind (charsets, lexicons, patterns): 0 = no array, or 1 and per page: 0 = no entry, or 1 and the regions' ids
//     -> resolve_region_opts() (rec_line_opts.h) of all pages: ok <per page charset:lexicon:pattern,.. or ->   or   error: <message>
//   lines <defaults> <counts> <n_pages> <boxes of each page> then 0 = the defaults, or 1 and every box's charset lexicon pattern
//     -> expand_line_opts() over pages whose first lines follow each other: any=c,l,p lines=charset:lexicon:pattern,..  or  error: ..
//   split <lanes> <active> <max_side_len> <nl> <n_pages> <h w of each page>
//     -> lanes_for(lanes, active, n_pages) then lane_split() of the pages over nl lanes (lane_split.h): <lanes_for> <first[0..nl]>
// (am_max != 0 sets the CTC-head statistics with am_tiles = gemm_argmax_tiles(Npad16); a_scale != 0 sets a scale and a row table)
#include "lane_split.h"
#include "nn.h"
#include "rec_tail_plan.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace rt;

static const char* kernel_name(nn::GemmKernel k) {
  switch (k) {
    case nn::GemmKernel::none: return "none";
    case nn::GemmKernel::invalid: return "invalid";
    case nn::GemmKernel::split: return "split";
    case nn::GemmKernel::w: return "w";
    case nn::GemmKernel::dma: return "dma";
    case nn::GemmKernel::wide_256x240: return "wide_256x240";
    case nn::GemmKernel::wide_128x240: return "wide_128x240";
    case nn::GemmKernel::wide_128x128: return "wide_128x128";
    case nn::GemmKernel::stream: return "stream";
    case nn::GemmKernel::narrow: return "narrow";
    case nn::GemmKernel::argmax_256x240: return "argmax_256x240";
    case nn::GemmKernel::argmax_128x128: return "argmax_128x128";
    case nn::GemmKernel::argmax_narrow: return "argmax_narrow";
  }
  return "?";
}

static void print_dw(const nn::DwPlan& p) {
  static const char* const names[] = {"invalid", "rows32", "rows64", "sweep"};
  printf("%s %d %d %d %d %d %u %u\n", names[(int)p.kernel], p.kernel == nn::DwKernel::sweep ? p.inst : 0, p.R, p.lanes, p.spb, p.chunks, p.grid_x, p.grid_z);
}

static void print_list(const char* name, const std::vector<int>& v) {
  printf(" %s=%s", name, v.empty() ? "-" : "");
  for (size_t i = 0; i < v.size(); i++) printf(i ? ",%d" : "%d", v[i]);
}
static void print_line(const lx::Line& l) { printf("%d:%d:%d:%d:%lld", l.row0, l.T, l.lex, l.slot, l.out); }
static void print_line(const pt::Line& l) { printf("%d:%d:%d:%d:%lld", l.row0, l.T, l.pat, l.slot, l.bp); }
template <typename Line>
static void print_lines(const char* name, const char* rows_name, const std::vector<Line>& lines, const std::vector<int>& rows) {
  printf(" %s=%s", name, lines.empty() ? "-" : "");
  for (size_t i = 0; i < lines.size(); i++) { if (i) printf(","); print_line(lines[i]); }
  print_list(rows_name, rows);
}
// n lists of a query as lx::Tables: n16 n32 n64 each, its entries of 1, 8 and 16 ids (class 1 throughout)
static void read_lists(std::istream& in, int n, lx::Tables& tb) {
  for (int k = 0; k < n && in; k++) {
    int n16, n32, n64;
    in >> n16 >> n32 >> n64;
    if (!in || n16 < 0 || n32 < 0 || n64 < 0) { in.setstate(std::ios::failbit); break; }
    std::vector<int32_t> lens;
    lens.insert(lens.end(), (size_t)n16, 1); lens.insert(lens.end(), (size_t)n32, 8); lens.insert(lens.end(), (size_t)n64, 16);
    size_t n_ids = 0;
    for (int32_t m : lens) n_ids += (size_t)m;
    const std::vector<int32_t> ids(n_ids, 1);
    tb.add(ids.data(), lens.data(), (int)lens.size());
  }
}
// an optional array of a query: a 0, or a 1 and n values
template <typename T>
static bool read_optional(std::istream& in, size_t n, std::vector<T>& v) {
  int has = 0;
  in >> has;
  v.assign(has ? n : 0, T());
  for (T& x : v) in >> x;
  return has != 0;
}

int main() {
  static float dummy_f[4];
  static int dummy_i[4];
  const int env_lc_wave = nn::g_lc_wave, env_dw_sweep = nn::g_dw_sweep;   // what RT_LC_WAVE / RT_DW_SWEEP selected
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    in >> op;
    if (op == "plan") {
      int cus, lda, K, N, Npad16, ldc, coff, am, res, asc;
      long long M;
      Epilogue e;
      in >> nn::g_gemm_variant >> nn::g_gemm_dma >> nn::g_gemm_split >> nn::g_argmax_wide >> cus >> lda >> M >> K >> N >> Npad16 >> ldc >>
          coff >> am >> res >> asc >> e.a_tab_stride >> e.act >> e.has_lab >> e.n_img >> e.ld_scale;
      if (!in) { printf("bad query\n"); return 2; }
      if (am) { e.am_max = dummy_f; e.am_idx = dummy_i; e.am_sum = dummy_f; e.am_tiles = nn::gemm_argmax_tiles(Npad16); }
      if (res) { e.residual = dummy_f; e.ld_res = ldc; }
      if (asc) { e.a_scale = dummy_f; e.a_tab = dummy_i; }
      const nn::GemmPlan p = nn::gemm_plan(lda, M, K, N, Npad16, ldc, coff, e, cus);
      printf("%s %d %d %d %d %u %u %s\n", kernel_name(p.kernel), p.nt, p.kg, (int)p.bf, (int)p.se, p.grid_x, p.grid_y,
             p.kernel == nn::GemmKernel::invalid ? p.error : p.label);
    } else if (op == "se_rows") {
      int lda, K, N, Npad16, act;
      long long M, min_pix;
      in >> nn::g_gemm_variant >> nn::g_gemm_dma >> nn::g_gemm_split >> lda >> M >> K >> N >> Npad16 >> act >> min_pix;
      if (!in) { printf("bad query\n"); return 2; }
      printf("%d\n", nn::gemm_se_rows(lda, M, K, N, Npad16, act, min_pix));
    } else if (op == "dw") {
      int dw_sweep, K, sh, sw, Cp, maxHo, maxWo, pooled;
      in >> dw_sweep >> K >> sh >> sw >> Cp >> maxHo >> maxWo >> pooled;
      if (!in) { printf("bad query\n"); return 2; }
      nn::g_dw_sweep = dw_sweep < 0 ? env_dw_sweep : dw_sweep;
      print_dw(nn::dw_plan(K, sh, sw, Cp, maxHo, maxWo, pooled != 0));
    } else if (op == "lc") {
      nn::LcShape s;
      Epilogue e;
      int lc_wave, dw_sweep, se, bias;
      in >> lc_wave >> dw_sweep >> s.K >> s.sh >> s.sw >> s.Cp >> s.C >> s.N >> s.Npad16 >> s.dw_act >> s.dw_has_lab >> se >> s.maxHo >>
          s.maxWo >> s.rows >> s.min_pix >> e.act >> e.has_lab >> bias;
      if (!in) { printf("bad query\n"); return 2; }
      nn::g_lc_wave = lc_wave < 0 ? env_lc_wave : lc_wave;
      nn::g_dw_sweep = dw_sweep < 0 ? env_dw_sweep : dw_sweep;
      s.se = se != 0; s.ldy = chan_pitch(s.N);
      if (bias) e.bias = dummy_f;
      const nn::LcPlan p = nn::lc_plan(s, e);
      static const char* const routes[] = {"unfused", "thin", "wave", "lds"};
      if (p.route != nn::LC_UNFUSED) printf("%s %d %d %u\n", routes[p.route], p.inst, p.tile_h, p.grid_x);
      else { printf("unfused %d ", p.se_rows); print_dw(p.dw); }
    } else if (op == "tail") {
      int l0, l1, cand_k, NL, n_lex = 0;
      in >> l0 >> l1 >> cand_k >> NL;
      if (!in || NL < 0 || l0 < 0 || l0 > l1 || l1 > NL) { printf("bad query\n"); return 2; }
      std::vector<long long> tok_off((size_t)NL + 1, 0);
      for (int i = 0; i < NL; i++) { int T; in >> T; tok_off[(size_t)i + 1] = tok_off[(size_t)i] + T; }
      std::vector<int> sets, lexs;
      std::vector<float> snaps;
      const bool has_set = read_optional(in, (size_t)NL, sets), has_lex = read_optional(in, (size_t)NL, lexs);
      in >> n_lex;
      lx::Tables tb;
      read_lists(in, n_lex, tb);
      const bool has_snap = read_optional(in, (size_t)n_lex, snaps);
      if (!in) { printf("bad query\n"); return 2; }
      for (int v : lexs) if (v < 0 || v > n_lex) { printf("bad query\n"); return 2; }
      const RecTailPlan p = rec_tail_plan(tok_off.data(), l0, l1, has_set ? sets.data() : nullptr, has_lex ? lexs.data() : nullptr, tb,
                                          has_snap ? snaps.data() : nullptr);
      printf("rows=%lld z5=%d has_lex=%d snap=%d table=%lld fits=%d max_waves=%d", p.rows, (int)p.needs_z5(cand_k), (int)p.has_lex(),
             (int)p.snap, p.table, (int)p.table_fits(), p.max_waves);
      print_list("row_set", p.row_set); print_list("crows", p.crows);
      print_lines("lines", "lrows", p.lines, p.lrows);
      printf("\n");
    } else if (op == "group" || op == "capacity") {
      int l0, l1, beam, nbest, NL, n_lex = 0, n_kw = 0, n_pat = 0;
      in >> l0 >> l1 >> beam >> nbest >> NL;
      if (!in || NL < 0 || l0 < 0 || l0 > l1 || l1 > NL) { printf("bad query\n"); return 2; }
      std::vector<long long> tok_off((size_t)NL + 1, 0);
      for (int i = 0; i < NL; i++) { int T; in >> T; tok_off[(size_t)i + 1] = tok_off[(size_t)i] + T; }
      lx::Tables tb, ktb;
      pt::Tables ptb;
      in >> n_lex;
      read_lists(in, n_lex, tb);
      std::vector<float> snaps((size_t)std::max(n_lex, 0));
      for (float& v : snaps) in >> v;
      in >> n_kw;
      read_lists(in, n_kw, ktb);
      in >> n_pat;
      for (int k = 0; k < n_pat && in; k++) { int S, P; in >> S >> P; ptb.pats.push_back(pt::Pat{S, P, 0, 0, 0, 0, 0}); }
      std::vector<RecLineOpts> opts((size_t)NL);
      for (RecLineOpts& o : opts) in >> o.charset >> o.lexicon >> o.pattern >> o.keywords;
      if (!in) { printf("bad query\n"); return 2; }
      for (const RecLineOpts& o : opts)
        if (o.lexicon < 0 || o.lexicon > n_lex || o.pattern < 0 || o.pattern > n_pat || o.keywords < 0 || o.keywords > n_kw) { printf("bad query\n"); return 2; }
      const RecTailPlan p = rec_tail_plan(tok_off.data(), l0, l1, opts.data(), RecStores{&tb, snaps.data(), &ptb, &ktb}, beam, nbest);
      if (op == "capacity") {
        const std::string why = p.refusal(beam);
        printf("%s\n", why.empty() ? "-" : why.c_str());
      } else {
        print_list("row_set", p.row_set); print_list("crows", p.crows);
        print_lines("lines", "lrows", p.lines, p.lrows); print_lines("plines", "prows", p.plines, p.prows);
        print_lines("klines", "krows", p.klines, p.krows); print_lines("blines", "brows", p.blines, p.brows);
        printf("\n");
      }
    } else if (op == "defaults") {
      RecLineOpts o;
      in >> o.charset >> o.lexicon >> o.pattern;
      if (!in) { printf("bad query\n"); return 2; }
      const std::string bad = rec_opts_conflict(o);
      printf("%s%s\n", bad.empty() ? "ok" : "error: ", bad.c_str());
    } else if (op == "regions" || op == "lines") {
      RecLineOpts dflt, counts;
      int n_pages = 0;
      in >> dflt.charset >> dflt.lexicon >> dflt.pattern >> counts.charset >> counts.lexicon >> counts.pattern >> n_pages;
      if (!in || n_pages < 0) { printf("bad query\n"); return 2; }
      std::vector<int> n((size_t)n_pages);
      for (int& x : n) in >> x;
      for (int x : n) if (!in || x < 0) { printf("bad query\n"); return 2; }
      std::string bad;
      if (op == "regions") {
        std::vector<std::vector<int>> vals[3];
        std::vector<const int*> ptrs[3];
        const int* const* ids[3] = {nullptr, nullptr, nullptr};
        for (int j = 0; j < 3; j++) {
          int has = 0;
          in >> has;
          if (!has) continue;
          vals[j].resize((size_t)n_pages); ptrs[j].assign((size_t)n_pages, nullptr);
          for (int i = 0; i < n_pages; i++)
            if (read_optional(in, (size_t)n[(size_t)i], vals[j][(size_t)i])) ptrs[j][(size_t)i] = vals[j][(size_t)i].data();
          ids[j] = ptrs[j].data();
        }
        if (!in) { printf("bad query\n"); return 2; }
        std::vector<std::vector<RecLineOpts>> out((size_t)n_pages);
        bad = resolve_region_opts(0, n_pages, n.data(), ids, dflt, counts, out);
        if (bad.empty()) {
          printf("ok");
          for (const auto& page : out) {
            printf(" %s", page.empty() ? "-" : "");
            for (size_t k = 0; k < page.size(); k++) printf("%s%d:%d:%d", k ? "," : "", page[k].charset, page[k].lexicon, page[k].pattern);
          }
        }
      } else {
        struct Page { int first_line, n_boxes; };
        std::vector<Page> pages((size_t)n_pages);
        int NL = 0, has = 0;
        for (int i = 0; i < n_pages; i++) { pages[(size_t)i] = {NL, n[(size_t)i]}; NL += n[(size_t)i]; }
        in >> has;
        std::vector<std::vector<RecLineOpts>> vals((size_t)n_pages);
        std::vector<const RecLineOpts*> ptrs;
        for (int i = 0; has && i < n_pages; i++) {
          vals[(size_t)i].resize((size_t)n[(size_t)i]);
          for (RecLineOpts& o : vals[(size_t)i]) in >> o.charset >> o.lexicon >> o.pattern;
          ptrs.push_back(vals[(size_t)i].data());
        }
        if (!in) { printf("bad query\n"); return 2; }
        std::vector<RecLineOpts> lines;
        RecLineAny any;
        bad = expand_line_opts(pages.data(), n_pages, NL, has ? ptrs.data() : nullptr, dflt, counts, lines, any);
        if (bad.empty()) {
          printf("any=%d,%d,%d lines=%s", (int)any.charset, (int)any.lexicon, (int)any.pattern, lines.empty() ? "-" : "");
          for (size_t k = 0; k < lines.size(); k++) printf("%s%d:%d:%d", k ? "," : "", lines[k].charset, lines[k].lexicon, lines[k].pattern);
        }
      }
      if (!bad.empty()) printf("error: %s", bad.c_str());
      printf("\n");
    } else if (op == "split") {
      int lanes, active, max_side_len, nl, n_pages = 0;
      in >> lanes >> active >> max_side_len >> nl >> n_pages;
      if (!in || nl < 1 || n_pages < 0) { printf("bad query\n"); return 2; }
      std::vector<int> hs((size_t)n_pages), ws((size_t)n_pages);
      for (int i = 0; i < n_pages; i++) in >> hs[(size_t)i] >> ws[(size_t)i];
      if (!in) { printf("bad query\n"); return 2; }
      printf("%d", lanes_for(lanes, active, n_pages));
      for (int f : lane_split(hs.data(), ws.data(), n_pages, max_side_len, nl)) printf(" %d", f);
      printf("\n");
    } else if (!op.empty()) {
      printf("unknown query %s\n", op.c_str());
      return 2;
    }
    fflush(stdout);
  }
  return 0;
}
