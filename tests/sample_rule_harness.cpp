// sample_rule_harness.cpp -- recur_amd/csrc/sample_rule.h under the host compiler alone, for tests/test_sample_rule.py: the
// rule k_texts_continue draws a text's next symbol by, asked on the CPU.  The exponential and the generator are the oracle's
// (liboracle.so: orc_fast_expf, orc_rand64, orc_init_rand64), passed to the rule as its functors.
//
//   sample_rule_harness BIAS SEED COUNT SCORE...      (scores as C hexadecimal floats, or "nan")
//
// draws COUNT symbols from the one row of scores with a generator seeded SEED and prints
//   picks=<pick>,<pick>,...      (-1: the draw met the attempt cap)
//   rng=<a>,<b>,<c>,<d>          the generator afterwards
//   draws=<n>                    the rand64 steps taken
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "sample_rule.h"

extern "C" {
struct OrcRng {
  unsigned long long a, b, c, d;
};
unsigned long long orc_rand64(OrcRng *x);
void orc_init_rand64(OrcRng *x, unsigned long long seed);
float orc_fast_expf(float x);
}

struct OracleExp {
  float operator()(float x) const { return orc_fast_expf(x); }
};
struct CountedRand64 {
  OrcRng *g;
  long draws;
  unsigned long long operator()() {
    draws++;
    return orc_rand64(g);
  }
};

int main(int argc, char **argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: %s BIAS SEED COUNT SCORE...\n", argv[0]);
    return 2;
  }
  const float bias = strtof(argv[1], nullptr);
  const unsigned long long seed = strtoull(argv[2], nullptr, 0);
  const int count = atoi(argv[3]);
  std::vector<float> score;
  for (int i = 4; i < argc; i++) {
    score.push_back(strtof(argv[i], nullptr));
  }
  const int n = (int)score.size();
  std::vector<float> p(n);
  OrcRng g;
  orc_init_rand64(&g, seed);
  CountedRand64 draw = {&g, 0};
  printf("picks=");
  for (int k = 0; k < count; k++) {
    int pick;
    if (bias >= SAMPLE_GREEDY_BIAS) {
      pick = sample_greedy(score.data(), n);
    } else {
      sample_distribution(p.data(), score.data(), n, bias, OracleExp{}, SampleSolo{});
      pick = sample_draw(p.data(), n, draw);
    }
    printf("%s%d", k ? "," : "", pick);
  }
  printf("\nrng=%llu,%llu,%llu,%llu\ndraws=%ld\n", g.a, g.b, g.c, g.d, draw.draws);
  return 0;
}
