// The rec pattern compiler (retto_amd/csrc/ctc_pattern.h) on mutated and random pattern bytes, built with AddressSanitizer and
// UBSan by tests/test_pattern_fuzz_cpu.py.  Every input must end in a status code; an accepted one in tables inside the caps whose
// host Viterbi, run on random logits at T = min_steps and min_steps - 1, matches exactly at the first and returns a path the DFA
// accepts.  Usage: fuzz_pattern ITERS SEED; prints "<accepted> accepted <rejected> rejected".
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../retto_amd/csrc/ctc_pattern.h"

using namespace rt;

static uint64_t g_state = 1;
static uint64_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return g_state; }
static int below(int n) { return (int)(rnd() % (uint64_t)n); }

#define REQUIRE(cond, what)                                                                  \
  do {                                                                                       \
    if (!(cond)) { fprintf(stderr, "fuzz_pattern: %s (input \"%s\")\n", what, text.c_str()); return false; } \
  } while (0)

static bool check_one(const std::vector<std::string>& dict, const std::string& text, bool* accepted) {
  pt::Compiled c;
  std::string err;
  const int rc = pt::compile(dict, text.data(), text.size(), c, err);
  *accepted = rc == pt::OK;
  if (rc != pt::OK) {
    REQUIRE(rc == pt::ERR_UTF8 || rc == pt::ERR_INVALID || rc == pt::ERR_CAPACITY, "an unknown status");
    REQUIRE(err.find("byte offset") != std::string::npos, "a message without its byte offset");
    return true;
  }
  const int N = (int)dict.size();
  REQUIRE(c.classes == N && c.S >= 1 && c.S <= pt::MAX_STATES && c.P >= 0 && c.P <= pt::MAX_PAIRS && c.G >= 1 && c.G <= N, "sizes outside the caps");
  REQUIRE(c.group_of.size() == (size_t)N && c.delta.size() == (size_t)c.S * c.G && c.accept.size() == (size_t)c.S, "table sizes");
  REQUIRE(c.min_steps >= 1 && c.min_steps <= 2 * c.S + 1, "min_steps");
  for (int v : c.group_of) REQUIRE(v >= 0 && v < c.G, "group_of");
  for (int v : c.delta) REQUIRE(v >= -1 && v < c.S, "delta");
  pt::Rule R;
  REQUIRE(R.build(N, c.S, c.G, c.group_of.data(), c.delta.data(), c.accept.data()).empty() && R.P == c.P, "the tables do not rebuild");
  for (int T = c.min_steps - 1; T <= c.min_steps; T++) {
    std::vector<float> logits((size_t)std::max(T, 1) * N), lse((size_t)std::max(T, 1), 0.0f), prob((size_t)std::max(T, 1));
    for (float& v : logits) v = (float)below(2001) / 100.0f - 10.0f;
    for (int t = 0; t < T; t++) lse[(size_t)t] = lx::row_lse(logits.data() + (size_t)t * N, N);
    std::vector<int32_t> idx((size_t)std::max(T, 1), -1);
    const pt::LineResult r = pt::viterbi_line(R, logits.data(), N, lse.data(), T, idx.data(), prob.data());
    REQUIRE(r.matched == (T == c.min_steps ? 1 : 0), "matched against min_steps");
    if (!r.matched) continue;
    int q = 0;
    for (int t = 0; t < T; t++) {
      const int k = idx[(size_t)t];
      REQUIRE(k >= 0 && k < N, "a class outside the dictionary");
      if (k == 0 || (t > 0 && k == idx[(size_t)t - 1])) continue;
      q = c.delta[(size_t)q * c.G + c.group_of[(size_t)k]];
      REQUIRE(q >= 0, "the path leaves the DFA");
    }
    REQUIRE(c.accept[(size_t)q] != 0, "the path ends outside the accepting states");
  }
  return true;
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 1000;
  g_state = 0x9E3779B97F4A7C15ull ^ (uint64_t)(argc > 2 ? atoll(argv[2]) : 1);
  std::vector<std::string> dict = {"blank"};
  for (char ch = '0'; ch <= '9'; ch++) dict.push_back(std::string(1, ch));
  for (char ch = 'a'; ch <= 'h'; ch++) dict.push_back(std::string(1, ch));
  for (char ch = 'A'; ch <= 'D'; ch++) dict.push_back(std::string(1, ch));
  for (const char* e : {"-", ".", ",", "a", "ab", "\xC3\xA9", "\xE4\xB8\xAD", "", "^", "]", "\\"}) dict.push_back(e);
  dict.push_back(" ");
  const std::vector<std::string> seeds = {
      "[0-9]{4}-[0-9]{2}-[0-9]{2}", "[0-9]{1,3}(,[0-9]{3})*\\.[0-9]{2}", "[A-D]{2}[0-9]{2} ?[A-D]{3}", "a|bc|def", "(ab|cb)*", "[a-h]*",
      "\\c{3}\\c{27}+", "[^0-9a]+\\d?", ".{2}", "a{63}", "a{64}", "(a?){5}b{2,}", "\xC3\xA9\xE4\xB8\xAD|\\^\\]\\\\", "[\\c{1}\\c{27}\\-.]*", "", "()|a",
      "((a{8}){8}){8}", "((a*){8}){8}", "[a-]"};
  const char alphabet[] = "\\.[]()|?*+{}^-,0123456789abcdhA D\xC3\xA9\xE4\xB8\xAD";
  long acc = 0, rej = 0;
  for (int it = 0; it < iters; it++) {
    std::string text = seeds[(size_t)below((int)seeds.size())];
    const int mode = below(8);
    if (mode == 0) {   // random bytes
      text.clear();
      for (int n = below(24); n > 0; n--) text.push_back((char)below(256));
    } else if (mode == 1) {   // random text over the alphabet
      text.clear();
      for (int n = below(40); n > 0; n--) text.push_back(alphabet[below((int)sizeof alphabet - 1)]);
    } else if (mode == 2) {   // two seeds spliced
      const std::string& o = seeds[(size_t)below((int)seeds.size())];
      text = text.substr(0, (size_t)below((int)text.size() + 1)) + o.substr((size_t)below((int)o.size() + 1));
    } else if (mode == 3 && it % 50 == 0) {   // long text, on both sides of MAX_BYTES
      std::string unit = text.empty() ? "a" : text;
      while ((int)text.size() < pt::MAX_BYTES - 8 + below(16)) text += unit[(size_t)below((int)unit.size())];
    } else {   // a few point mutations
      for (int n = 1 + below(3); n > 0; n--) {
        const int at = below((int)text.size() + 1), op = below(3);
        const char ch = below(4) ? alphabet[below((int)sizeof alphabet - 1)] : (char)below(256);
        if (op == 0 || text.empty()) text.insert(text.begin() + at, ch);
        else if (op == 1) text[(size_t)std::min(at, (int)text.size() - 1)] = ch;
        else text.erase(text.begin() + std::min(at, (int)text.size() - 1));
      }
    }
    bool ok = false;
    if (!check_one(dict, text, &ok)) return 1;
    (ok ? acc : rej)++;
  }
  printf("%ld accepted %ld rejected\n", acc, rej);
  return 0;
}
