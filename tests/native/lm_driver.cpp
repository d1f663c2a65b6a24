// Host-only driver for the rec language model (retto_amd/csrc/ctc_lm.h) and the host beam rule with fusion (ctc_host_ref.h),
// compiled with g++ -fsanitize=address,undefined by tests/test_lm_driver_cpu.py and run as a program: no GPU, nothing loaded into
// Python.  Every array is exactly sized, so the sanitizer sees every index the parser, the compiler, the walk and the rule touch.
//   lm_driver arpa DICT ARPA OOV_LOG10
//     the ARPA file compiled over the dictionary file (one entry per line; the blank first and the space last are added here)
//     -> one line: rc=.. n=.. ids=.. order=.. dropped=.. states=.. arcs=.. start=.. oov=.. msg=..
//   lm_driver fuzz DICT ARPA OOV_LOG10 SEED ROUNDS
//     the file truncated at ROUNDS places and with 1 .. 4 bytes changed ROUNDS times (a fixed generator from SEED), each compiled
//     and, where it compiles, walked over strings of every class -> one line: ok=.. refused=.. (refusals must carry a message)
//   lm_driver beam IN OUT
//     IN: int32 N, n_lines, beam, nbest, n, then float32 oov, alpha, beta, then tokens_per_line [n_lines], ngram_lens [n], ngram_ids,
//     logp [n], backoff [n], z5 [rows][120], W [120][N], bias [N], then the initial counts [n_lines], beams [n_lines][nbest] (2 words
//     each), tokens [rows * nbest], lm [n_lines][nbest] (2 words each).  hr::BeamLmArgs' check and hr::beam_lm_ref on them
//     -> OUT: the four outputs in that order; stdout: "ok" or "error: <message>"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "ctc_host_ref.h"

using namespace rt;

static std::string slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
static std::vector<std::string> dictionary(const char* path) {
  std::vector<std::string> d(1, "blank");
  const std::string s = slurp(path);
  for (size_t pos = 0; pos < s.size();) {
    size_t e = s.find('\n', pos);
    if (e == std::string::npos) e = s.size();
    d.push_back(s.substr(pos, e - pos));
    pos = e + 1;
  }
  d.push_back(" ");
  return d;
}
// (exactly sized copy: the parser gets no byte past the text)
static int compile_text(const std::vector<std::string>& d, const std::string& text, float oov_log10, lm::Ids& f, lm::Model& m, std::string& msg) {
  std::vector<char> exact(text.begin(), text.end());
  return lm::compile_arpa(d, exact.data(), exact.size(), oov_log10, f, m, msg);
}

int main(int argc, char** argv) {
  const std::string op = argc > 1 ? argv[1] : "";
  if (op == "arpa" && argc == 5) {
    const std::vector<std::string> d = dictionary(argv[2]);
    lm::Ids f; lm::Model m; std::string msg;
    const int rc = compile_text(d, slurp(argv[3]), (float)atof(argv[4]), f, m, msg);
    printf("rc=%d n=%d ids=%zu order=%d dropped=%d states=%zu arcs=%zu start=%d oov=%.9g msg=%s\n", rc, rc ? 0 : m.n_ngrams, rc ? (size_t)0 : f.ids.size(),
           rc ? 0 : m.order, rc ? 0 : m.dropped, rc ? (size_t)0 : m.states.size(), rc ? (size_t)0 : m.arcs.size(), rc ? 0 : m.start, rc ? 0.0 : (double)m.oov, msg.c_str());
    return 0;
  }
  if (op == "fuzz" && argc == 7) {
    const std::vector<std::string> d = dictionary(argv[2]);
    const std::string text = slurp(argv[3]);
    const float oov = (float)atof(argv[4]);
    uint64_t x = strtoull(argv[5], nullptr, 10) * 2862933555777941757ull + 3037000493ull;
    auto next = [&]() { x = x * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(x >> 33); };
    const int rounds = atoi(argv[6]);
    int ok = 0, refused = 0;
    auto one = [&](const std::string& t) {
      lm::Ids f; lm::Model m; std::string msg;
      const int rc = compile_text(d, t, oov, f, m, msg);
      if (rc != lm::OK) {
        if (msg.empty()) { printf("a refusal without a message\n"); exit(1); }
        refused++;
        return;
      }
      ok++;
      const lm::View v = m.view();
      std::vector<int32_t> s(12);
      for (int r = 0; r < 8; r++) {
        for (int32_t& c : s) c = 1 + (int32_t)(next() % (uint32_t)(m.classes - 1));
        (void)lm::walk(v, s.data(), (int)s.size());
      }
      for (int c = 1; c < m.classes; c++)
        for (int q = 0; q < (int)m.states.size(); q++) (void)lm::step(v, q, c);
    };
    for (int r = 0; r < rounds; r++) one(text.substr(0, text.empty() ? 0 : next() % text.size()));
    static const char repl[] = "\t\n \\-0123456789.e<>s/=abgmnrkuNIF\xff";
    for (int r = 0; r < rounds && !text.empty(); r++) {
      std::string t = text;
      for (int k = 1 + (int)(next() % 4); k > 0; k--) t[next() % t.size()] = repl[next() % (sizeof repl - 1)];
      one(t);
    }
    printf("ok=%d refused=%d\n", ok, refused);
    return 0;
  }
  if (op == "beam" && argc == 4) {
    const std::string in = slurp(argv[2]);
    size_t at = 0;
    auto take = [&](void* dst, size_t bytes) {
      if (at + bytes > in.size()) { printf("short input\n"); exit(1); }
      memcpy(dst, in.data() + at, bytes);
      at += bytes;
    };
    int32_t h[5];
    float w[3];
    take(h, sizeof h); take(w, sizeof w);
    const int N = h[0], n_lines = h[1], beam = h[2], nbest = h[3], n = h[4];
    if (N < 0 || n_lines < 0 || nbest < 0 || n < 0) { printf("short input\n"); return 1; }
    std::vector<int32_t> tpl((size_t)n_lines), lens((size_t)n);
    take(tpl.data(), tpl.size() * 4); take(lens.data(), lens.size() * 4);
    long long rows = 0, n_ids = 0;
    for (int32_t t : tpl) rows += t > 0 ? t : 0;
    for (int32_t l : lens) n_ids += l > 0 ? l : 0;
    std::vector<int32_t> ids((size_t)n_ids);
    std::vector<float> logp((size_t)n), bo((size_t)n), z((size_t)rows * hr::HEAD_D), W((size_t)hr::HEAD_D * N), b((size_t)N);
    take(ids.data(), ids.size() * 4); take(logp.data(), logp.size() * 4); take(bo.data(), bo.size() * 4);
    take(z.data(), z.size() * 4); take(W.data(), W.size() * 4); take(b.data(), b.size() * 4);
    std::vector<int32_t> counts((size_t)n_lines), tokens((size_t)rows * nbest);
    std::vector<rt_beam> beams((size_t)n_lines * nbest);
    std::vector<rt_beam_lm> lms((size_t)n_lines * nbest);
    take(counts.data(), counts.size() * 4); take(beams.data(), beams.size() * 8); take(tokens.data(), tokens.size() * 4); take(lms.data(), lms.size() * 8);
    hr::BeamLmArgs a;
    static_cast<hr::Head&>(a) = hr::Head{z.data(), W.data(), b.data(), N, tpl.data(), n_lines};
    a.beam = beam; a.nbest = nbest; a.counts_out = counts.data(); a.beams_out = beams.data(); a.tokens_out = tokens.data();
    a.ids = {ids.data(), lens.data(), logp.data(), bo.data(), n, w[0]}; a.alpha = w[1]; a.beta = w[2]; a.lm_out = lms.data();
    const std::string bad = a.error();
    if (bad.empty()) hr::beam_lm_ref(a);
    std::ofstream out(argv[3], std::ios::binary);
    out.write((const char*)counts.data(), (std::streamsize)(counts.size() * 4)); out.write((const char*)beams.data(), (std::streamsize)(beams.size() * 8));
    out.write((const char*)tokens.data(), (std::streamsize)(tokens.size() * 4)); out.write((const char*)lms.data(), (std::streamsize)(lms.size() * 8));
    printf("%s%s\n", bad.empty() ? "ok" : "error: ", bad.c_str());
    return 0;
  }
  printf("usage: lm_driver arpa|fuzz|beam ...\n");
  return 2;
}
