// Host-only driver for the keyword part of rt::rec_tail_plan (retto_amd/csrc/rec_tail_plan.h) and the four-kind rules of
// rec_line_opts.h, compiled with g++ by tests/test_keyword_plan_cpu.py: no GPU.  One query per input line:
//   plan l0 l1 cand_k n_lines T.. n_kw (n n16 n32).. has_kw [kw..]
//     list k has n entries, n16 / n32 of them in the 16- / 32-lane buckets (the plan reads nothing else of it)
//     -> rows=.. z5=.. has_kw=.. ktable=.. fits=.. kmax_waves=.. klines=row0:T:list:slot:out,.. krows=..
//   regions <4 defaults> <4 counts> n_pages n_quads.. then per kind (charset, lexicon, pattern, keywords): 0, or 1 and per page
//     "-" (null) or n_quads ids
//     -> resolve_region_opts() over the four kinds: ok <per page charset:lexicon:pattern:keywords,.. or ->   or   error: <message>
//   lines <4 defaults> <4 counts> n_pages n_boxes.. has_opts [per line charset lexicon pattern keywords]
//     -> expand_line_opts(): any=c,l,p,k lines=charset:lexicon:pattern:keywords,..   or   error: <message>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "rec_tail_plan.h"

using namespace rt;

static void read4(std::istream& in, RecLineOpts& o) { in >> o.charset >> o.lexicon >> o.pattern >> o.keywords; }
static void print4(const RecLineOpts& o, bool comma) {
  printf("%s%d:%d:%d:%d", comma ? "," : "", o.charset, o.lexicon, o.pattern, o.keywords);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    in >> op;
    if (op == "plan") {
      int l0, l1, cand_k, n, n_kw, has;
      in >> l0 >> l1 >> cand_k >> n;
      std::vector<long long> off((size_t)n + 1, 0);
      for (int i = 0; i < n; i++) { long long T; in >> T; off[(size_t)i + 1] = off[(size_t)i] + T; }
      in >> n_kw;
      lx::Tables tb;
      for (int k = 0, first = 0; k < n_kw; k++) {
        int m, n16, n32;
        in >> m >> n16 >> n32;
        tb.lex.push_back(lx::Lex{first, m, n16, n32});
        first += m;
      }
      in >> has;
      std::vector<int> kws((size_t)n, 0);
      for (int i = 0; has && i < n; i++) in >> kws[(size_t)i];
      if (!in) { printf("bad query\n"); continue; }
      const RecTailPlan p = rec_tail_plan(off.data(), l0, l1, nullptr, nullptr, lx::Tables(), nullptr, nullptr, nullptr,
                                          has ? kws.data() : nullptr, &tb);
      printf("rows=%lld z5=%d has_kw=%d ktable=%lld fits=%d kmax_waves=%d klines=", p.rows, (int)p.needs_z5(cand_k), (int)p.has_kw(),
             p.ktable, (int)p.ktable_fits(), p.kmax_waves);
      if (p.klines.empty()) printf("-");
      for (size_t i = 0; i < p.klines.size(); i++)
        printf("%s%d:%d:%d:%d:%lld", i ? "," : "", p.klines[i].row0, p.klines[i].T, p.klines[i].lex, p.klines[i].slot, p.klines[i].out);
      printf(" krows=");
      if (p.krows.empty()) printf("-");
      for (size_t i = 0; i < p.krows.size(); i++) printf("%s%d", i ? "," : "", p.krows[i]);
      printf(" other=%d%d%d\n", (int)p.has_lex(), (int)p.has_pat(), (int)!p.crows.empty());
    } else if (op == "regions" || op == "lines") {
      RecLineOpts dflt, counts;
      int n_pages = 0;
      read4(in, dflt); read4(in, counts);
      in >> n_pages;
      if (!in || n_pages < 0) { printf("bad query\n"); continue; }
      std::vector<int> n((size_t)n_pages);
      for (int& x : n) in >> x;
      std::string bad;
      if (op == "regions") {
        std::vector<std::vector<int>> vals[REC_N_KINDS];
        std::vector<const int*> ptrs[REC_N_KINDS];
        const int* const* ids[REC_N_KINDS] = {nullptr, nullptr, nullptr, nullptr};
        for (int j = 0; j < REC_N_KINDS; j++) {
          int has = 0;
          in >> has;
          if (!has) continue;
          vals[j].resize((size_t)n_pages); ptrs[j].assign((size_t)n_pages, nullptr);
          for (int i = 0; i < n_pages; i++) {
            std::string tok;
            for (int k = 0; k < n[(size_t)i]; k++) {
              in >> tok;
              if (tok == "-") break;   // (a null page entry: one "-" for the whole page)
              vals[j][(size_t)i].push_back(std::stoi(tok));
            }
            if (n[(size_t)i] == 0) in >> tok;   // ("-" or "." for a page without regions)
            if ((int)vals[j][(size_t)i].size() == n[(size_t)i] && tok != "-") ptrs[j][(size_t)i] = vals[j][(size_t)i].data();
          }
          ids[j] = ptrs[j].data();
        }
        if (!in) { printf("bad query\n"); continue; }
        std::vector<std::vector<RecLineOpts>> out((size_t)n_pages);
        bad = resolve_region_opts(0, n_pages, n.data(), ids, REC_N_KINDS, dflt, counts, out);
        if (bad.empty()) {
          printf("ok");
          for (const auto& page : out) {
            printf(" %s", page.empty() ? "-" : "");
            for (size_t k = 0; k < page.size(); k++) print4(page[k], k > 0);
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
          for (RecLineOpts& o : vals[(size_t)i]) read4(in, o);
          ptrs.push_back(vals[(size_t)i].data());
        }
        if (!in) { printf("bad query\n"); continue; }
        std::vector<RecLineOpts> lines;
        RecLineAny any;
        bad = expand_line_opts(pages.data(), n_pages, NL, has ? ptrs.data() : nullptr, dflt, counts, lines, any);
        if (bad.empty()) {
          printf("any=%d,%d,%d,%d lines=%s", (int)any.charset, (int)any.lexicon, (int)any.pattern, (int)any.keywords, lines.empty() ? "-" : "");
          for (size_t k = 0; k < lines.size(); k++) print4(lines[k], k > 0);
        }
      }
      if (!bad.empty()) printf("error: %s", bad.c_str());
      printf("\n");
    } else if (!op.empty()) {
      printf("unknown query %s\n", op.c_str());
    }
    fflush(stdout);
  }
  return 0;
}
