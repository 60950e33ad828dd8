// fast_exp_rule_harness.cpp -- recur_amd/csrc/fast_exp_rule.h under the host compiler alone, for tests/test_fast_exp_rule.py:
// the exponential every loss kernel and the host's sampler call, asked on the CPU.
//
//   fast_exp_rule_harness values FILE     float32 values; prints for each "BITS ROUNDS": fast_expf_rounds' value as the bits
//                                         of a float32 and its number of scaling rounds; fast_expf itself must give the
//                                         same bits (exit status 3 where it does not)
//   fast_exp_rule_harness sweep STRIDE    every STRIDE-th positive finite float in ascending order and FLT_MAX, each with
//                                         its negative; prints "MAX_ROUNDS DESCENTS ASKED": the largest number of rounds, how
//                                         often a larger |x| took fewer rounds than a smaller one, or the two signs of one
//                                         |x| differed (the count is a function of |x| that never falls), and how many
//                                         values were asked
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "fast_exp_rule.h"

static unsigned bits(float x) {
  unsigned u;
  memcpy(&u, &x, sizeof u);
  return u;
}

static float from_bits(unsigned u) {
  float x;
  memcpy(&x, &u, sizeof x);
  return x;
}

static bool same(float a, float b) { return bits(a) == bits(b) || (a != a && b != b); }

int main(int argc, char **argv) {
  const std::string what = argc > 1 ? argv[1] : "";
  if (what == "values" && argc == 3) {
    FILE *f = fopen(argv[2], "rb");
    if (!f) {
      perror(argv[2]);
      return 1;
    }
    float x;
    while (fread(&x, sizeof x, 1, f) == 1) {
      int rounds = -1;
      const float a = fast_expf_rounds(x, &rounds);
      if (!same(a, fast_expf(x))) {
        fprintf(stderr, "fast_expf and fast_expf_rounds differ at the float with bits %u\n", bits(x));
        return 3;
      }
      printf("%u %d\n", bits(a), rounds);
    }
    fclose(f);
    return 0;
  }
  if (what == "sweep" && argc == 3) {
    const unsigned long stride = strtoul(argv[2], nullptr, 0);
    const unsigned last = 0x7f7fffffu; /* FLT_MAX */
    if (stride == 0) {
      return 2;
    }
    int largest = 0, before = 0;
    unsigned long descents = 0, asked = 0;
    for (unsigned long u = 0;; u += stride) {
      if (u > last) {
        u = last;
      }
      int up = -1, down = -1;
      (void)fast_expf_rounds(from_bits((unsigned)u), &up);
      (void)fast_expf_rounds(from_bits((unsigned)u | 0x80000000u), &down);
      descents += (up < before) + (up != down);
      before = up;
      largest = up > largest ? up : largest;
      asked += 2;
      if (u == last) {
        break;
      }
    }
    printf("%d %lu %lu\n", largest, descents, asked);
    return 0;
  }
  fprintf(stderr, "usage: %s values FILE | sweep STRIDE\n", argv[0]);
  return 2;
}
