// dream_rule_harness.cpp -- recur_amd/csrc/dream_rule.h under the host compiler alone, for tests/test_dream_rule.py and the
// host side of tests/test_gpu_dream_sequences.py: the rule k_dream_step turns a net's answer into its next input by, asked
// on the CPU.  The generator is the oracle's (liboracle.so: orc_cheap_gaussian_noise), passed to the rule as its functor.
//
//   dream_rule_harness tanh FILE                    float32 values; prints dream_tanh of each as the bits of a float32
//   dream_rule_harness next NOISE FILE              float32 pairs (a, g); prints dream_next(a, NOISE, g) as bits
//   dream_rule_harness rows NOISE ROWS N RAW RNG OUT
//        one launch of the kernel for ROWS rows of N outputs: RAW holds the raw outputs [ROWS][N] float32, RNG the rows'
//        generators [ROWS][4] uint64.  Writes OUT.frame (dream_tanh of every output), OUT.next (dream_next of those, the
//        draws made per row in index order; with NOISE 0 nothing is drawn) and OUT.rng (the generators afterwards).
// NOISE is a C hexadecimal float.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "dream_rule.h"

extern "C" {
struct OrcRng {
  unsigned long long a, b, c, d;
};
float orc_cheap_gaussian_noise(OrcRng *x);
}

struct OracleGaussian {
  OrcRng *g;
  float operator()() { return orc_cheap_gaussian_noise(g); }
};

template <class T>
static std::vector<T> slurp(const char *path) {
  FILE *f = fopen(path, "rb");
  if (!f) {
    perror(path);
    exit(1);
  }
  std::vector<T> v;
  T x;
  while (fread(&x, sizeof x, 1, f) == 1) {
    v.push_back(x);
  }
  fclose(f);
  return v;
}

template <class T>
static void spill(const std::string &path, const std::vector<T> &v) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f || fwrite(v.data(), sizeof(T), v.size(), f) != v.size() || fclose(f)) {
    perror(path.c_str());
    exit(1);
  }
}

static unsigned bits(float x) {
  unsigned u;
  memcpy(&u, &x, sizeof u);
  return u;
}

int main(int argc, char **argv) {
  const std::string what = argc > 1 ? argv[1] : "";
  if (what == "tanh" && argc == 3) {
    for (float x : slurp<float>(argv[2])) {
      printf("%u\n", bits(dream_tanh(x)));
    }
    return 0;
  }
  if (what == "next" && argc == 4) {
    const float noise = strtof(argv[2], nullptr);
    const std::vector<float> v = slurp<float>(argv[3]);
    for (size_t i = 0; i + 1 < v.size(); i += 2) {
      printf("%u\n", bits(dream_next(v[i], noise, v[i + 1])));
    }
    return 0;
  }
  if (what == "rows" && argc == 8) {
    const float noise = strtof(argv[2], nullptr);
    const size_t rows = strtoul(argv[3], nullptr, 0), n = strtoul(argv[4], nullptr, 0);
    const std::vector<float> raw = slurp<float>(argv[5]);
    std::vector<unsigned long long> words = slurp<unsigned long long>(argv[6]);
    if (raw.size() != rows * n || words.size() != rows * 4) {
      fprintf(stderr, "%zu outputs and %zu generator words for %zu rows of %zu\n", raw.size(), words.size(), rows, n);
      return 1;
    }
    std::vector<float> frame(rows * n), next(rows * n), gz(n);
    for (size_t k = 0; k < rows; k++) {
      OrcRng g = {words[4 * k], words[4 * k + 1], words[4 * k + 2], words[4 * k + 3]};
      if (dream_draws(noise)) {
        OracleGaussian gaussian = {&g};
        dream_draw(gz.data(), (int)n, 1, gaussian);
      }
      for (size_t i = 0; i < n; i++) {
        const float a = dream_tanh(raw[k * n + i]);
        frame[k * n + i] = a;
        next[k * n + i] = dream_draws(noise) ? dream_next(a, noise, gz[i]) : a;
      }
      words[4 * k] = g.a;
      words[4 * k + 1] = g.b;
      words[4 * k + 2] = g.c;
      words[4 * k + 3] = g.d;
    }
    const std::string out = argv[7];
    spill(out + ".frame", frame);
    spill(out + ".next", next);
    spill(out + ".rng", words);
    return 0;
  }
  fprintf(stderr, "usage: %s tanh FILE | next NOISE FILE | rows NOISE ROWS N RAW RNG OUT\n", argv[0]);
  return 2;
}
