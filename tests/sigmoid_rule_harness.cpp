// sigmoid_rule_harness.cpp -- recur_amd/csrc/sigmoid_rule.h under a host compiler alone, for tests/test_sigmoid_rule.py:
//   sigmoid_rule_harness COUNT IN OUT    IN holds COUNT raw outputs then COUNT targets (float32); writes OUT.answer
//                                        (sigmoid_answer with fast_exp_rule.h's fast_expf, the exponential the kernels
//                                        run), OUT.error and OUT.loss (sigmoid_error, sigmoid_loss of the answers)
// Built with -ffp-contract=off; also built with -fsanitize=address,undefined and run as it is.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "sigmoid_rule.h"

struct HostExp {
  float operator()(float x) const { return fast_expf(x); }
};

static bool write_floats(const std::string &path, const std::vector<float> &v) {
  FILE *f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = std::fwrite(v.data(), sizeof(float), v.size(), f) == v.size();
  return std::fclose(f) == 0 && ok;
}

int main(int argc, char **argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: sigmoid_rule_harness COUNT IN OUT\n");
    return 2;
  }
  const long count = std::atol(argv[1]);
  if (count < 0) return 2;
  std::vector<float> in(2 * (size_t)count), answer((size_t)count), error((size_t)count), loss((size_t)count);
  FILE *f = std::fopen(argv[2], "rb");
  if (!f || std::fread(in.data(), sizeof(float), in.size(), f) != in.size()) {
    std::fprintf(stderr, "%s: not %ld pairs\n", argv[2], count);
    return 1;
  }
  std::fclose(f);
  for (long i = 0; i < count; i++) {
    const float a = sigmoid_answer(in[(size_t)i], HostExp{});
    const float t = in[(size_t)(count + i)];
    answer[(size_t)i] = a;
    error[(size_t)i] = sigmoid_error(a, t);
    loss[(size_t)i] = sigmoid_loss(a, t);
  }
  const std::string out = argv[3];
  if (!write_floats(out + ".answer", answer) || !write_floats(out + ".error", error) || !write_floats(out + ".loss", loss)) {
    std::perror(argv[3]);
    return 1;
  }
  return 0;
}
