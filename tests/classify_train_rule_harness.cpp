// classify_train_rule_harness.cpp -- recur_amd/csrc/classify_train_rule.h under the host compiler alone, for
// tests/test_classify_train_rule.py: what rnn_amd_set_classify_steps decides on the host per generation, the gate its loss
// kernels write, its refusals and the balanced-training choice, asked on the CPU.
//
//   classify_train_rule_harness decisions T N G SIZES GEN0 TARGETS
//       SIZES: the group sizes, comma separated; GEN0: every stream's generation counter before the block; TARGETS: a file
//       of T * N * G int32.  One line: the T masks, classify_mask_stride(N) bytes each; the T active counts; the N
//       generation counters; the trained groups of the block
//   classify_train_rule_harness gate BITS...        a float's bits each -> 0 or 1 each
//   classify_train_rule_harness refusal HAVE_FEATURES HAVE_TARGETS N_STEPS LD INPUT_SIZE N_GROUPS OFFSETS SIZES OUTPUT_SIZE
//       OFFSETS, SIZES: comma separated, or - for NULL.  <code> <text>
//   classify_train_rule_harness probabilities BIAS SEEN       BIAS a float's bits, SEEN comma separated -> the floats' bits
//   classify_train_rule_harness choose GENERATIONS N G OFFSETS SIZES N_OUTPUTS BIAS TARGETS DRAWS
//       TARGETS: a file of GENERATIONS * N * G int32; DRAWS: a file of uint64, the generator's output in order; BIAS a
//       float's bits, or - for "every label trains".  Per generation one line: the N * G entries of use, the N flags, the
//       groups trained; then a last line: seen, used (N_OUTPUTS each) and the draws taken
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "classify_train_rule.h"

template <class T> static std::vector<T> read_file(const char *path) {
  std::vector<T> data;
  FILE *f = fopen(path, "rb");
  if (!f) {
    perror(path);
    exit(2);
  }
  T buf[1024];
  size_t n;
  while ((n = fread(buf, sizeof(T), 1024, f)) > 0) {
    data.insert(data.end(), buf, buf + n);
  }
  fclose(f);
  return data;
}

static std::vector<int> list_of(const char *text) {
  std::vector<int> out;
  if (!strcmp(text, "-") || !*text) {
    return out;
  }
  const char *p = text;
  for (;;) {
    char *end;
    out.push_back((int)strtol(p, &end, 10));
    if (*end != ',') {
      break;
    }
    p = end + 1;
  }
  return out;
}

static float float_of_bits(const char *text) {
  const unsigned bits = (unsigned)strtoul(text, nullptr, 10);
  float x;
  memcpy(&x, &bits, sizeof x);
  return x;
}

static unsigned bits_of(float x) {
  unsigned bits;
  memcpy(&bits, &x, sizeof bits);
  return bits;
}

struct Draws {
  const std::vector<uint64_t> *from;
  size_t taken;
};
static uint64_t next_draw(void *ctx) {
  Draws *d = static_cast<Draws *>(ctx);
  if (d->taken >= d->from->size()) {
    fprintf(stderr, "more draws than the file holds\n");
    exit(2);
  }
  return (*d->from)[d->taken++];
}

int main(int argc, char **argv) {
  const char *mode = argc > 1 ? argv[1] : "";
  if (!strcmp(mode, "decisions") && argc == 8) {
    const int T = atoi(argv[2]), n = atoi(argv[3]), G = atoi(argv[4]);
    const std::vector<int> sizes = list_of(argv[5]);
    const std::vector<int> targets = read_file<int>(argv[7]);
    if ((int)sizes.size() != G || targets.size() != (size_t)T * n * G) {
      fprintf(stderr, "%zu sizes and %zu targets are not this block's\n", sizes.size(), targets.size());
      return 2;
    }
    const size_t stride = classify_mask_stride(n);
    std::vector<unsigned char> masks(T * stride, 0xaa); /* (the rule clears the padding itself) */
    std::vector<int> active(T, -1);
    std::vector<unsigned> generation(n, (unsigned)strtoul(argv[6], nullptr, 10));
    const long long trained = classify_block_decisions(targets.data(), T, n, G, sizes.data(), masks.data(), active.data(),
                                                       generation.data());
    for (unsigned char m : masks) printf("%d ", m);
    for (int a : active) printf("%d ", a);
    for (unsigned g : generation) printf("%u ", g);
    printf("%lld\n", trained);
    return 0;
  }
  if (!strcmp(mode, "gate") && argc > 2) {
    for (int i = 2; i < argc; i++) printf("%d ", classify_gate_raises(float_of_bits(argv[i])));
    printf("\n");
    return 0;
  }
  if (!strcmp(mode, "refusal") && argc == 11) {
    const std::vector<int> offsets = list_of(argv[8]), sizes = list_of(argv[9]);
    const int code = classify_block_refusal(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]),
                                            strcmp(argv[8], "-") ? offsets.data() : nullptr,
                                            strcmp(argv[9], "-") ? sizes.data() : nullptr, atoi(argv[10]));
    printf("%d %s\n", code, classify_block_refusal_text(code));
    return 0;
  }
  if (!strcmp(mode, "probabilities") && argc == 4) {
    const std::vector<int> seen_i = list_of(argv[3]);
    const std::vector<uint32_t> seen(seen_i.begin(), seen_i.end());
    std::vector<float> p(seen.size());
    classify_balance_probabilities(seen.data(), (int)seen.size(), float_of_bits(argv[2]), p.data());
    for (float x : p) printf("%u ", bits_of(x));
    printf("\n");
    return 0;
  }
  if (!strcmp(mode, "choose") && argc == 11) {
    const int gens = atoi(argv[2]), n = atoi(argv[3]), G = atoi(argv[4]), n_out = atoi(argv[7]);
    const std::vector<int> offsets = list_of(argv[5]), sizes = list_of(argv[6]);
    const bool balanced = strcmp(argv[8], "-") != 0;
    const float bias = balanced ? float_of_bits(argv[8]) : 0.0f;
    const std::vector<int> targets = read_file<int>(argv[9]);
    const std::vector<uint64_t> file = read_file<uint64_t>(argv[10]);
    if ((int)offsets.size() != G || (int)sizes.size() != G || targets.size() != (size_t)gens * n * G) {
      return 2;
    }
    Draws draws = {&file, 0};
    std::vector<uint32_t> seen(n_out, 0), used(n_out, 0);
    std::vector<float> p(n_out);
    std::vector<int> use((size_t)n * G);
    std::vector<unsigned char> trains(n);
    for (int t = 0; t < gens; t++) {
      classify_balance_probabilities(seen.data(), n_out, bias, p.data());
      const int k = classify_balance_choose(n, G, offsets.data(), sizes.data(), targets.data() + (size_t)t * n * G,
                                            balanced ? p.data() : nullptr, seen.data(), used.data(), next_draw, &draws, use.data(),
                                            trains.data());
      for (int u : use) printf("%d ", u);
      for (unsigned char f : trains) printf("%d ", f);
      printf("%d\n", k);
    }
    for (uint32_t s : seen) printf("%u ", s);
    for (uint32_t u : used) printf("%u ", u);
    printf("%zu\n", draws.taken);
    return 0;
  }
  fprintf(stderr, "see the head of tests/classify_train_rule_harness.cpp\n");
  return 2;
}
