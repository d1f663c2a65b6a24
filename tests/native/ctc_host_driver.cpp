// Host-only driver for the rec CTC tail's host references and their checks (retto_amd/csrc/ctc_host_ref.h), compiled with g++
// under AddressSanitizer + UBSan by tests/test_ctc_host_driver_cpu.py: no GPU, no library.  usage: ctc_host_driver IN OUT
// IN, 32-bit little-endian words: kind (0 candidates, 1 charset, 2 lexicon, 3 pattern, 4 keywords, 5 beam), N, n_lines, the lines'
// time steps, the number of arrays, then each array as its word count (-1: a null pointer) and its words (int32 or float32 bits).
// The arrays of a kind, in order ("params": its int32 scalars):
//   candidates  params {K}                  z5 W bias idx prob
//   charset     params {K, n_sets}          z5 W bias idx prob line_set masks
//   lexicon     params {n_lex, align}       z5 W bias line_lex entry_ids entry_lens first_entry  [align: lex_min_post idx prob]
//   pattern     params {n_pat}              z5 W bias line_pat pat_S pat_G group_of delta accept idx prob
//   keywords    params {n_kw}               z5 W bias line_kw entry_ids entry_lens first_entry kw_min_score
//   beam        params {beam, nbest}        z5 W bias
// OUT: the word 1 and the check's message, or the word 0 and every output array (count, words) in the order of the host entry's
// signature (idx / prob, where the kind rewrites them, first).  Outputs start as zeros, as the test hands them to the library.
// The check sees output pointers of zero words; they get their sizes from the rows and the table the check wrote.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "ctc_host_ref.h"

using namespace rt;

namespace {

struct Array { bool null = true; std::vector<uint32_t> w; };
struct Case {
  int kind = 0, N = 0;
  std::vector<int32_t> tpl;
  std::vector<Array> arr;
  int param(size_t i) const { return (int)arr.at(0).w.at(i); }
  template <class T> T* at(size_t i) { Array& a = arr.at(i); return a.null ? nullptr : reinterpret_cast<T*>(a.w.data()); }
  const float* f(size_t i) { return at<const float>(i); }
  const int32_t* i(size_t i) { return at<const int32_t>(i); }
};

bool read_words(FILE* f, void* p, size_t n) { return fread(p, 4, n, f) == n; }
bool read_case(const char* path, Case& c) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  int32_t head[3], n_arrays = 0;
  bool ok = read_words(f, head, 3) && head[2] >= 0 && head[2] < 4096;
  if (ok) { c.kind = head[0]; c.N = head[1]; c.tpl.resize((size_t)head[2]); ok = read_words(f, c.tpl.data(), c.tpl.size()); }
  ok = ok && read_words(f, &n_arrays, 1) && n_arrays >= 1 && n_arrays < 64;
  for (int k = 0; ok && k < n_arrays; k++) {
    int32_t n = 0;
    Array a;
    ok = read_words(f, &n, 1) && n >= -1 && n < (1 << 24);
    if (ok && n >= 0) { a.null = false; a.w.resize((size_t)n); ok = read_words(f, a.w.data(), a.w.size()); }
    c.arr.push_back(std::move(a));
  }
  fclose(f);
  return ok;
}

// The outputs of a call, in order.  Before the check every output is an allocation of no words (not null, and any access is the
// sanitizer's to report); size() then gives it its words, zeroed, or the words the call hands in.
struct Outputs {
  std::vector<std::unique_ptr<uint32_t[]>> p;
  std::vector<size_t> n;
  template <class T> T* add() { p.emplace_back(new uint32_t[0]); n.push_back(0); return reinterpret_cast<T*>(p.back().get()); }
  template <class T> T* size(size_t k, long long words, const void* init = nullptr) {
    p[k].reset(new uint32_t[(size_t)words]());
    n[k] = (size_t)words;
    if (init) memcpy(p[k].get(), init, (size_t)words * 4);
    return reinterpret_cast<T*>(p[k].get());
  }
  bool write(FILE* f) const {
    for (size_t k = 0; k < p.size(); k++) {
      const int32_t cnt = (int32_t)n[k];
      if (fwrite(&cnt, 4, 1, f) != 1 || fwrite(p[k].get(), 4, n[k], f) != n[k]) return false;
    }
    return true;
  }
};

hr::Head head_of(Case& c) { return hr::Head{c.f(1), c.f(2), c.f(3), c.N, c.tpl.data(), (int)c.tpl.size()}; }

// each: fill the struct, check it, size the outputs, run the reference; returns the check's message
std::string run_candidates(Case& c, Outputs& o) {
  hr::CandArgs a{head_of(c)};
  a.idx = c.i(4); a.prob = c.f(5); a.K = c.param(0);
  a.cands_out = o.add<rt_candidate>(); a.cols_out = o.add<int32_t>(); a.n_tokens_out = o.add<int32_t>();
  if (!a.ok()) return "bad argument";
  a.cands_out = o.size<rt_candidate>(0, a.rows * a.K * 2); a.cols_out = o.size<int32_t>(1, a.rows); a.n_tokens_out = o.size<int32_t>(2, a.n_lines);
  hr::candidates_ref(a);
  return std::string();
}
std::string run_charset(Case& c, Outputs& o) {
  hr::CharsetArgs a{head_of(c)};
  a.K = c.param(0); a.n_sets = c.param(1);
  a.idx = c.at<int32_t>(4); a.prob = c.at<float>(5); a.line_set = c.i(6); a.masks = c.at<const uint32_t>(7);
  o.add<int32_t>(); o.add<float>();
  a.tokens_out = o.add<int32_t>(); a.n_tokens_out = o.add<int32_t>(); a.scores_out = o.add<float>();
  a.cands_out = o.add<rt_candidate>(); a.cols_out = o.add<int32_t>();
  if (!a.ok()) return "bad argument";
  a.idx = o.size<int32_t>(0, a.rows, a.idx); a.prob = o.size<float>(1, a.rows, a.prob);
  a.tokens_out = o.size<int32_t>(2, a.rows); a.n_tokens_out = o.size<int32_t>(3, a.n_lines); a.scores_out = o.size<float>(4, a.n_lines);
  a.cands_out = a.K > 0 ? o.size<rt_candidate>(5, a.rows * a.K * 2) : nullptr; a.cols_out = a.K > 0 ? o.size<int32_t>(6, a.rows) : nullptr;
  hr::charset_ref(a);
  return std::string();
}
std::string run_lexicon(Case& c, Outputs& o) {
  hr::LexiconArgs a{head_of(c)};
  a.line_lex = c.i(4); a.lists = {c.i(5), c.i(6), c.i(7), c.param(0)};
  a.align = c.param(1) != 0;
  if (a.align) {
    a.lex_min_post = c.f(8); a.idx = c.at<int32_t>(9); a.prob = c.at<float>(10);
    o.add<int32_t>(); o.add<float>(); a.snapped_out = o.add<int32_t>(); a.vit_out = o.add<float>();
  }
  const size_t k0 = o.p.size();
  a.loglik_out = o.add<float>(); a.matches_out = o.add<rt_lexicon_match>(); a.n_matches_out = o.add<int32_t>();
  const std::string bad = a.error();
  if (!bad.empty()) return bad;
  if (a.align) {
    a.idx = o.size<int32_t>(0, a.rows, a.idx); a.prob = o.size<float>(1, a.rows, a.prob);
    a.snapped_out = o.size<int32_t>(2, a.n_lines); a.vit_out = o.size<float>(3, a.n_lines);
  }
  a.loglik_out = o.size<float>(k0, a.table); a.matches_out = o.size<rt_lexicon_match>(k0 + 1, (long long)a.n_lines * RT_LEXICON_MATCHES * 3);
  a.n_matches_out = o.size<int32_t>(k0 + 2, a.n_lines);
  hr::lexicon_ref(a);
  return std::string();
}
std::string run_pattern(Case& c, Outputs& o) {
  hr::PatternArgs a{head_of(c)};
  a.n_pat = c.param(0);
  a.line_pat = c.i(4); a.pat_S = c.i(5); a.pat_G = c.i(6); a.group_of = c.i(7); a.delta = c.i(8); a.accept = c.i(9);
  a.idx = c.at<int32_t>(10); a.prob = c.at<float>(11);
  o.add<int32_t>(); o.add<float>();
  a.matched_out = o.add<int32_t>(); a.vit_out = o.add<float>(); a.logprob_out = o.add<float>(); a.free_out = o.add<float>();
  const std::string bad = a.error();
  if (!bad.empty()) return bad;
  a.idx = o.size<int32_t>(0, a.rows, a.idx); a.prob = o.size<float>(1, a.rows, a.prob);
  a.matched_out = o.size<int32_t>(2, a.n_lines); a.vit_out = o.size<float>(3, a.n_lines);
  a.logprob_out = o.size<float>(4, a.n_lines); a.free_out = o.size<float>(5, a.n_lines);
  hr::pattern_ref(a);
  return std::string();
}
std::string run_keywords(Case& c, Outputs& o) {
  hr::KeywordArgs a{head_of(c)};
  a.line_kw = c.i(4); a.lists = {c.i(5), c.i(6), c.i(7), c.param(0)}; a.kw_min_score = c.f(8);
  a.score_out = o.add<float>(); a.span_out = o.add<int32_t>(); a.hits_out = o.add<rt_keyword_hit>(); a.n_hits_out = o.add<int32_t>();
  const std::string bad = a.error();
  if (!bad.empty()) return bad;
  a.score_out = o.size<float>(0, a.table); a.span_out = o.size<int32_t>(1, 2 * a.table);
  a.hits_out = o.size<rt_keyword_hit>(2, (long long)a.n_lines * RT_KEYWORD_HITS * 12); a.n_hits_out = o.size<int32_t>(3, a.n_lines);
  hr::keywords_ref(a);
  return std::string();
}
std::string run_beam(Case& c, Outputs& o) {
  hr::BeamArgs a{head_of(c)};
  a.beam = c.param(0); a.nbest = c.param(1);
  a.counts_out = o.add<int32_t>(); a.beams_out = o.add<rt_beam>(); a.tokens_out = o.add<int32_t>();
  const std::string bad = a.error();
  if (!bad.empty()) return bad;
  a.counts_out = o.size<int32_t>(0, a.n_lines); a.beams_out = o.size<rt_beam>(1, (long long)a.n_lines * a.nbest * 2);
  a.tokens_out = o.size<int32_t>(2, a.rows * a.nbest);
  hr::beam_ref(a);
  return std::string();
}

}  // namespace

static_assert(sizeof(rt_candidate) == 8 && sizeof(rt_lexicon_match) == 12 && sizeof(rt_keyword_hit) == 48 && sizeof(rt_beam) == 8,
              "the records' sizes in words, as the outputs are sized above");

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: ctc_host_driver IN OUT\n"); return 2; }
  Case c;
  if (!read_case(argv[1], c) || c.arr.at(0).null) { fprintf(stderr, "bad case file\n"); return 2; }
  std::string (*const run[])(Case&, Outputs&) = {run_candidates, run_charset, run_lexicon, run_pattern, run_keywords, run_beam};
  if (c.kind < 0 || c.kind > 5) { fprintf(stderr, "unknown kind %d\n", c.kind); return 2; }
  Outputs o;
  const std::string bad = run[c.kind](c, o);
  FILE* f = fopen(argv[2], "wb");
  if (!f) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
  const int32_t refused = bad.empty() ? 0 : 1;
  bool ok = fwrite(&refused, 4, 1, f) == 1;
  if (refused) ok = ok && fwrite(bad.data(), 1, bad.size(), f) == bad.size();
  else ok = ok && o.write(f);
  ok = fclose(f) == 0 && ok;
  return ok ? 0 : 2;
}
