// Host-only driver for the rec tail's text front end (retto_amd/csrc/rec_text.h): the dictionary loader and the charset, lexicon
// and vocabulary compilers, compiled with g++ -fsanitize=address,undefined by tests/test_rec_text_driver_cpu.py and run as a
// program: no GPU, nothing loaded into Python.  Both files are copied into exactly sized heap buffers, so the sanitizer sees
// every byte index the decoder, the line reader and the compilers touch, a read past the end included.
//   rec_text_driver dict DICT
//     -> rc=.. classes=.. msg=..            then one line: every entry in hex, "-" for an empty one
//   rec_text_driver charset DICT TEXT
//     -> rc=.. classes=.. msg=..            then one line: the mask's words
//   rec_text_driver lexicon DICT TEXT
//     -> rc=.. classes=.. msg=..            then two lines: the ids, the entries' lengths
//   rec_text_driver vocab DICT TEXT FLAGS
//     -> rc=.. classes=.. words=.. nodes=.. word_classes=.. variants_dropped=.. msg=..     then two lines: the ids, the words' lengths
// As the library's rt_debug_*_compile hooks: the dictionary is parsed first, classes stays 0 where it does not parse, and a
// refusal carries its code and message with no array behind it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "rec_text.h"

using namespace rt;

// a file's bytes in a heap block of exactly their number
struct Exact {
  std::unique_ptr<char[]> p; size_t n = 0;
  explicit Exact(const char* path) {
    std::ifstream f(path, std::ios::binary);
    const std::string s((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    n = s.size(); p.reset(new char[n]);
    if (n) memcpy(p.get(), s.data(), n);
  }
};
template <class T>
static void print_row(const std::vector<T>& v) {
  for (size_t i = 0; i < v.size(); i++) printf("%s%lld", i ? " " : "", (long long)v[i]);
  printf("\n");
}

int main(int argc, char** argv) {
  const std::string op = argc > 1 ? argv[1] : "";
  const bool known = (op == "dict" && argc == 3) || ((op == "charset" || op == "lexicon") && argc == 4) || (op == "vocab" && argc == 5);
  if (!known) { printf("usage: rec_text_driver dict|charset|lexicon|vocab DICT [TEXT [FLAGS]]\n"); return 2; }
  const Exact d(argv[2]);
  int rc = RT_OK, classes = 0;
  std::string msg, extra;
  std::vector<std::string> dict;
  std::vector<uint32_t> mask;
  std::vector<int32_t> ids, lens;
  try {
    dict = load_dictionary(std::vector<uint8_t>(d.p.get(), d.p.get() + d.n));
    classes = (int)dict.size();
    if (op != "dict") {
      const Exact t(argv[3]);
      if (op == "charset") mask = compile_charset(dict, t.p.get(), t.n, nullptr, 0);
      if (op == "lexicon") compile_lexicon(dict, t.p.get(), t.n, nullptr, nullptr, 0, ids, lens);
      if (op == "vocab") {
        vc::Ids f;
        const vc::Vocab m = compile_vocab(dict, t.p.get(), t.n, nullptr, nullptr, 0, atoi(argv[4]), f);
        ids = f.ids; lens = f.lens;
        extra = " words=" + std::to_string(m.n_words) + " nodes=" + std::to_string(m.nodes.size()) + " word_classes=" +
                std::to_string(m.n_word_classes) + " variants_dropped=" + std::to_string(m.variants_dropped);
      }
    }
  } catch (const RtError& e) {
    rc = e.code; msg = e.what();
    dict.clear(); mask.clear(); ids.clear(); lens.clear();
  }
  if (op == "vocab" && extra.empty()) extra = " words=0 nodes=0 word_classes=0 variants_dropped=0";
  printf("rc=%d classes=%d%s msg=%s\n", rc, classes, extra.c_str(), msg.c_str());
  if (op == "dict") {
    for (size_t i = 0; i < dict.size(); i++) {
      if (i) printf(" ");
      if (dict[i].empty()) printf("-");
      for (unsigned char c : dict[i]) printf("%02x", c);
    }
    printf("\n");
  } else if (op == "charset") {
    print_row(mask);
  } else {
    print_row(ids); print_row(lens);
  }
  return 0;
}
