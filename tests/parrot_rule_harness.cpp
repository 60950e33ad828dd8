// parrot_rule_harness.cpp -- recur_amd/csrc/parrot_rule.h under a host compiler alone, for tests/test_parrot_rule.py:
//   parrot_rule_harness pairs COUNT IN OUT    IN holds COUNT answers then COUNT targets (float32); writes OUT.error and
//                                             OUT.loss (parrot_error, parrot_loss of every pair)
//   parrot_rule_harness raw COUNT IN OUT      IN holds COUNT raw outputs then COUNT targets; writes OUT.answer
//                                             (dream_tanh), OUT.error and OUT.loss of the answers
//   parrot_rule_harness block HAVE_FRAMES N_STEPS LD INPUT_SIZE N OUTPUT_SIZE
//                                             prints parrot_block_refusal's code and its text: which blocks of frames
//                                             rnn_amd_set_dense_steps_tanh takes, asked without a device
// Built with -ffp-contract=off; also built with -fsanitize=address,undefined and run as it is.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "parrot_rule.h"

static bool write_floats(const std::string &path, const std::vector<float> &v) {
  FILE *f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = std::fwrite(v.data(), sizeof(float), v.size(), f) == v.size();
  return std::fclose(f) == 0 && ok;
}

int main(int argc, char **argv) {
  if (argc == 8 && !std::strcmp(argv[1], "block")) {
    const int code = parrot_block_refusal(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]),
                                          std::atoi(argv[6]), std::atoi(argv[7]));
    std::printf("%d %s\n", code, parrot_block_refusal_text(code));
    return 0;
  }
  if (argc != 5 || (std::strcmp(argv[1], "pairs") && std::strcmp(argv[1], "raw"))) {
    std::fprintf(stderr, "usage: parrot_rule_harness pairs|raw COUNT IN OUT\n");
    return 2;
  }
  const bool raw = !std::strcmp(argv[1], "raw");
  const long count = std::atol(argv[2]);
  if (count < 0) return 2;
  std::vector<float> in(2 * (size_t)count), answer((size_t)count), error((size_t)count), loss((size_t)count);
  FILE *f = std::fopen(argv[3], "rb");
  if (!f || std::fread(in.data(), sizeof(float), in.size(), f) != in.size()) {
    std::fprintf(stderr, "%s: not %ld pairs\n", argv[3], count);
    return 1;
  }
  std::fclose(f);
  for (long i = 0; i < count; i++) {
    const float a = raw ? dream_tanh(in[(size_t)i]) : in[(size_t)i];
    const float t = in[(size_t)(count + i)];
    answer[(size_t)i] = a;
    error[(size_t)i] = parrot_error(a, t);
    loss[(size_t)i] = parrot_loss(a, t);
  }
  const std::string out = argv[4];
  if ((raw && !write_floats(out + ".answer", answer)) || !write_floats(out + ".error", error) ||
      !write_floats(out + ".loss", loss)) {
    std::perror(argv[4]);
    return 1;
  }
  return 0;
}
