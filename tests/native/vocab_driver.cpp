// Host-only driver for the rec vocabulary (retto_amd/csrc/ctc_vocab.h) and the host beam rule with a word list (ctc_host_ref.h),
// compiled with g++ -fsanitize=address,undefined by tests/test_vocab_driver_cpu.py and run as a program: no GPU, nothing loaded
// into Python.  Every array is exactly sized, so the sanitizer sees every index the compiler, the walk and the rule touch.
//   vocab_driver words IN
//     IN: int32 classes, n, then word_lens [n], then the ids (the sum of the positive lengths).  vc::compile on them
//     -> one line: rc=.. words=.. nodes=.. arcs=.. word_classes=.. msg=..
//   vocab_driver fuzz CLASSES SEED ROUNDS
//     ROUNDS seeded id forms (a fixed generator from SEED), about half of them malformed -- an id that is the blank, negative or
//     >= classes, a length of 0, below 0 or above the limit, no word -- each compiled and, where it compiles, walked over strings
//     of every class and stepped from every state, the states outside the trie included -> one line: ok=.. refused=.. (refusals
//     must carry a message and a code)
//   vocab_driver beam IN OUT
//     IN: int32 N, n_lines, beam, nbest, n, n_words, then float32 oov, alpha, beta, gamma, then tokens_per_line [n_lines], ngram_lens
//     [n], word_lens [n_words], ngram_ids, logp [n], backoff [n], word_ids, z5 [rows][120], W [120][N], bias [N], then the initial
//     counts [n_lines], beams [n_lines][nbest] (2 words each), tokens [rows * nbest], lm [n_lines][nbest], vocab [n_lines][nbest] (2
//     words each).  hr::BeamVocabArgs' check and hr::beam_vocab_ref on them -> OUT: the five outputs in that order; stdout: "ok" or
//     "error: <message>"
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
struct Reader {
  std::string in; size_t at = 0;
  void take(void* dst, size_t bytes) {
    if (at + bytes > in.size()) { printf("short input\n"); exit(1); }
    if (bytes) memcpy(dst, in.data() + at, bytes);
    at += bytes;
  }
};

int main(int argc, char** argv) {
  const std::string op = argc > 1 ? argv[1] : "";
  if (op == "words" && argc == 3) {
    Reader r{slurp(argv[2])};
    int32_t h[2];
    r.take(h, sizeof h);
    if (h[1] < 0) { printf("short input\n"); return 1; }
    std::vector<int32_t> lens((size_t)h[1]);
    r.take(lens.data(), lens.size() * 4);
    long long n_ids = 0;
    for (int32_t l : lens) n_ids += l > 0 ? l : 0;
    std::vector<int32_t> ids((size_t)n_ids);
    r.take(ids.data(), ids.size() * 4);
    vc::Vocab m; std::string msg;
    const int rc = vc::compile(h[0], ids.data(), lens.data(), h[1], m, msg);
    printf("rc=%d words=%d nodes=%zu arcs=%zu word_classes=%d msg=%s\n", rc, rc ? 0 : m.n_words, rc ? (size_t)0 : m.nodes.size(),
           rc ? (size_t)0 : m.arcs.size(), rc ? 0 : m.n_word_classes, msg.c_str());
    return 0;
  }
  if (op == "fuzz" && argc == 5) {
    const int classes = atoi(argv[2]);
    uint64_t x = strtoull(argv[3], nullptr, 10) * 2862933555777941757ull + 3037000493ull;
    auto next = [&]() { x = x * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(x >> 33); };
    const int rounds = atoi(argv[4]);
    int ok = 0, refused = 0;
    for (int r = 0; r < rounds; r++) {
      const int fault = next() % 2 ? (int)(next() % 7) : -1;
      const int n = fault == 6 ? 0 : 1 + (int)(next() % 40);
      std::vector<int32_t> lens((size_t)n), ids;
      const int at = n ? (int)(next() % (uint32_t)n) : 0;
      for (int i = 0; i < n; i++) {
        int len = 1 + (int)(next() % (next() % 8 ? 6 : vc::MAX_LEN));
        if (i == at && fault == 3) len = 0;
        if (i == at && fault == 4) len = -(int)(next() % 5) - 1;
        if (i == at && fault == 5) len = vc::MAX_LEN + 1 + (int)(next() % 3);
        lens[(size_t)i] = len;
        for (int k = 0; k < len; k++) ids.push_back(1 + (int32_t)(next() % (uint32_t)(classes - 1)) % (next() % 3 ? 4 : classes - 1));   // (small ids often: shared prefixes)
        if (i == at && len > 0 && fault >= 0 && fault <= 2) ids.back() = fault == 0 ? 0 : fault == 1 ? -1 - (int32_t)(next() % 9) : classes + (int32_t)(next() % 9);
      }
      vc::Vocab m; std::string msg;
      const int rc = vc::compile(classes, ids.data(), lens.data(), n, m, msg);
      if (rc != vc::OK) {
        if (msg.empty() || (rc != vc::ERR_INVALID && rc != vc::ERR_CAPACITY)) { printf("a refusal without a message or a code\n"); return 1; }
        if (fault < 0) { printf("a well-formed vocabulary refused: %s\n", msg.c_str()); return 1; }
        refused++;
        continue;
      }
      if (fault >= 0) { printf("fault %d accepted\n", fault); return 1; }
      ok++;
      const vc::View v = m.view();
      std::vector<int32_t> s(24);
      for (int q = 0; q < 8; q++) {
        for (int32_t& c : s) c = 1 + (int32_t)(next() % (uint32_t)(classes - 1));
        const vc::Walk w = vc::walk(v, s.data(), (int)s.size());
        if (w.oov < 0 || w.closed < w.oov || w.closed > w.oov + 1 || w.state < vc::OFF || w.state >= v.n_nodes) { printf("a walk left its range\n"); return 1; }
      }
      const int states[] = {vc::OFF, -7, v.n_nodes, v.n_nodes + 5, 0x7fffffff};
      for (int c = 0; c <= classes; c++) {
        for (int q = 0; q < v.n_nodes; q++) (void)vc::step(v, q, c);
        for (int q : states) {
          const vc::Step t = vc::step(v, q, c);
          if (c >= 1 && c < classes && vc::is_word_class(v, c) && (t.next != vc::OFF || t.add != 0)) { printf("a state outside the trie is not OFF\n"); return 1; }
          (void)vc::close(v, q);
        }
      }
    }
    printf("ok=%d refused=%d\n", ok, refused);
    return 0;
  }
  if (op == "beam" && argc == 4) {
    Reader r{slurp(argv[2])};
    int32_t h[6];
    float w[4];
    r.take(h, sizeof h); r.take(w, sizeof w);
    const int N = h[0], n_lines = h[1], beam = h[2], nbest = h[3], n = h[4], n_words = h[5];
    if (N < 0 || n_lines < 0 || nbest < 0 || n < 0 || n_words < 0) { printf("short input\n"); return 1; }
    std::vector<int32_t> tpl((size_t)n_lines), lens((size_t)n), wlens((size_t)n_words);
    r.take(tpl.data(), tpl.size() * 4); r.take(lens.data(), lens.size() * 4); r.take(wlens.data(), wlens.size() * 4);
    long long rows = 0, n_ids = 0, n_wids = 0;
    for (int32_t t : tpl) rows += t > 0 ? t : 0;
    for (int32_t l : lens) n_ids += l > 0 ? l : 0;
    for (int32_t l : wlens) n_wids += l > 0 ? l : 0;
    std::vector<int32_t> ids((size_t)n_ids), wids((size_t)n_wids);
    std::vector<float> logp((size_t)n), bo((size_t)n), z((size_t)rows * hr::HEAD_D), W((size_t)hr::HEAD_D * N), b((size_t)N);
    r.take(ids.data(), ids.size() * 4); r.take(logp.data(), logp.size() * 4); r.take(bo.data(), bo.size() * 4); r.take(wids.data(), wids.size() * 4);
    r.take(z.data(), z.size() * 4); r.take(W.data(), W.size() * 4); r.take(b.data(), b.size() * 4);
    std::vector<int32_t> counts((size_t)n_lines), tokens((size_t)rows * nbest);
    std::vector<rt_beam> beams((size_t)n_lines * nbest);
    std::vector<rt_beam_lm> lms((size_t)n_lines * nbest);
    std::vector<rt_beam_vocab> vocs((size_t)n_lines * nbest);
    r.take(counts.data(), counts.size() * 4); r.take(beams.data(), beams.size() * 8); r.take(tokens.data(), tokens.size() * 4);
    r.take(lms.data(), lms.size() * 8); r.take(vocs.data(), vocs.size() * 8);
    hr::BeamVocabArgs a;
    static_cast<hr::Head&>(a) = hr::Head{z.data(), W.data(), b.data(), N, tpl.data(), n_lines};
    a.beam = beam; a.nbest = nbest; a.counts_out = counts.data(); a.beams_out = beams.data(); a.tokens_out = tokens.data();
    a.ids = {ids.data(), lens.data(), logp.data(), bo.data(), n, w[0]}; a.alpha = w[1]; a.beta = w[2]; a.lm_out = lms.data();
    a.words = {wids.data(), wlens.data(), n_words}; a.gamma = w[3]; a.vocab_out = vocs.data();
    const std::string bad = a.error();
    if (bad.empty()) hr::beam_vocab_ref(a);
    std::ofstream out(argv[3], std::ios::binary);
    out.write((const char*)counts.data(), (std::streamsize)(counts.size() * 4)); out.write((const char*)beams.data(), (std::streamsize)(beams.size() * 8));
    out.write((const char*)tokens.data(), (std::streamsize)(tokens.size() * 4)); out.write((const char*)lms.data(), (std::streamsize)(lms.size() * 8));
    out.write((const char*)vocs.data(), (std::streamsize)(vocs.size() * 8));
    printf("%s%s\n", bad.empty() ? "ok" : "error: ", bad.c_str());
    return 0;
  }
  printf("usage: vocab_driver words|fuzz|beam ...\n");
  return 2;
}
