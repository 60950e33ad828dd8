// automaton_rule_harness.cpp -- recur_amd/csrc/automaton_rule.h under the host compiler alone, for
// tests/test_automaton_rule.py: the rule k_automaton_step makes rnnca's next frame by, asked on the CPU.  The exponential
// is the oracle's (liboracle.so: orc_fast_expf), passed to the level rule as its functor.
//
//   automaton_rule_harness source W H EDGES REACH
//       for every cell (cy, then cx) and every offset (dy, then dx) in [-REACH, REACH]^2: the source cell; with EDGES 0 an
//       offset the single wrap does not bring back prints -1 and is not asked (`rawsource`: it is asked all the same)
//   automaton_rule_harness inputs W H EDGES LEN_POS PATTERN FRAME
//       FRAME: a file of 3 * W * H bytes.  For every cell its input row, the floats' bits as unsigned integers
//   automaton_rule_harness level FILE     FILE: float32 outputs.  Their levels
//   automaton_rule_harness byte FILE      FILE: float32 scaled values.  Their bytes
//   automaton_rule_harness pattern STRING MAX_PAIRS
//       rc=<0 | -1>, y=<dx>,<dy>;... and c=... as far as the lists got; the arrays have exactly MAX_PAIRS pairs of room
// One line of numbers separated by blanks, except for `pattern`.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "automaton_rule.h"

extern "C" float orc_fast_expf(float x);

struct OracleExp {
  float operator()(float x) const { return orc_fast_expf(x); }
};
struct FrameLevels {
  const unsigned char *frame;
  int cells;
  unsigned char operator()(int plane, int cell) const { return frame[(size_t)plane * cells + cell]; }
};

static std::vector<unsigned char> read_file(const char *path) {
  std::vector<unsigned char> data;
  FILE *f = fopen(path, "rb");
  if (!f) {
    perror(path);
    exit(2);
  }
  unsigned char buf[4096];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) {
    data.insert(data.end(), buf, buf + n);
  }
  fclose(f);
  return data;
}

static std::vector<float> read_floats(const char *path) {
  const std::vector<unsigned char> raw = read_file(path);
  std::vector<float> x(raw.size() / sizeof(float));
  memcpy(x.data(), raw.data(), x.size() * sizeof(float));
  return x;
}

static void print_list(const char *name, const int *o, int n) {
  printf("%s=", name);
  for (int i = 0; i < n; i++) {
    printf("%s%d,%d", i ? ";" : "", o[2 * i], o[2 * i + 1]);
  }
  printf("\n");
}

int main(int argc, char **argv) {
  const char *mode = argc > 1 ? argv[1] : "";
  if ((!strcmp(mode, "source") || !strcmp(mode, "rawsource")) && argc == 6) {
    const int w = atoi(argv[2]), h = atoi(argv[3]), edges = atoi(argv[4]), reach = atoi(argv[5]);
    const bool raw = mode[0] == 'r';
    for (int cy = 0; cy < h; cy++)
      for (int cx = 0; cx < w; cx++)
        for (int dy = -reach; dy <= reach; dy++)
          for (int dx = -reach; dx <= reach; dx++)
            printf("%d ", !raw && !edges && !automaton_wrap_reaches(dx, dy, w, h) ? -1
                                                                                   : automaton_source_cell(dx, dy, cx, cy, w, h, edges));
    printf("\n");
    return 0;
  }
  if (!strcmp(mode, "inputs") && argc == 8) {
    const int w = atoi(argv[2]), h = atoi(argv[3]), edges = atoi(argv[4]), len_pos = atoi(argv[5]);
    const int room = 8 * (int)strlen(argv[6]) + 1;
    std::vector<int> oy(2 * room), oc(2 * room);
    int ny = 0, nc = 0;
    if (automaton_parse_offsets(argv[6], oy.data(), &ny, oc.data(), &nc, room)) {
      return 3;
    }
    const std::vector<unsigned char> frame = read_file(argv[7]);
    if (frame.size() != 3 * (size_t)w * h) {
      fprintf(stderr, "%s: %zu bytes are no frame of %d x %d\n", argv[7], frame.size(), w, h);
      return 2;
    }
    const AutomatonRule g = {w, h, oy.data(), ny, oc.data(), nc, len_pos, edges};
    const FrameLevels level = {frame.data(), w * h};
    for (int cy = 0; cy < h; cy++)
      for (int cx = 0; cx < w; cx++)
        for (int i = 0; i < automaton_input_size(&g); i++) {
          const float x = automaton_input(g, cx, cy, i, level);
          unsigned bits;
          memcpy(&bits, &x, sizeof bits);
          printf("%u ", bits);
        }
    printf("\n");
    return 0;
  }
  if (!strcmp(mode, "level") && argc == 3) {
    for (float x : read_floats(argv[2])) {
      printf("%d ", (int)automaton_level(x, OracleExp{}));
    }
    printf("\n");
    return 0;
  }
  if (!strcmp(mode, "byte") && argc == 3) {
    for (float x : read_floats(argv[2])) {
      printf("%d ", (int)automaton_byte(x));
    }
    printf("\n");
    return 0;
  }
  if (!strcmp(mode, "pattern") && argc == 4) {
    const int room = atoi(argv[3]);
    int *oy = (int *)malloc(2 * (size_t)room * sizeof(int) + 1); /* exactly the room: a sanitizer sees a pair too many */
    int *oc = (int *)malloc(2 * (size_t)room * sizeof(int) + 1);
    int ny = -1, nc = -1;
    const int rc = automaton_parse_offsets(argv[2], oy, &ny, oc, &nc, room);
    printf("rc=%d\n", rc);
    print_list("y", oy, ny);
    print_list("c", oc, nc);
    free(oy);
    free(oc);
    return 0;
  }
  fprintf(stderr, "see the head of tests/automaton_rule_harness.cpp\n");
  return 2;
}
