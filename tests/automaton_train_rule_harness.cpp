// automaton_train_rule_harness.cpp -- recur_amd/csrc/automaton_train_rule.h under the host compiler alone, for
// tests/test_automaton_train_rule.py: what k_automaton_train_rows gathers for rnnca's trainers, the momentum of a
// generation and the refusals of rnn_amd_set_automaton_steps, asked on the CPU.
//
//   automaton_train_rule_harness block W H EDGES LEN_POS PATTERN T N PER_STEP FILM XY
//       FILM: a file of (T + 1) * 3 * W * H bytes; XY: a file of (PER_STEP ? T : 1) * N * 2 int32.  The rows
//       [T][N][input_size], then the targets [T][N][3], the floats' bits as unsigned integers, walked as the kernel walks them
//   automaton_train_rule_harness momentum GENERATION MOMENTUM SOFT_START      (hexadecimal floats) the momentum's bits
//   automaton_train_rule_harness refusals
//       a table of blocks, one line each: <name>=<code> <text>
// One line of numbers separated by blanks, except for `refusals`.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "automaton_train_rule.h"

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

static void print_bits(float x) {
  unsigned bits;
  memcpy(&bits, &x, sizeof bits);
  printf("%u ", bits);
}

// what rnn_amd_set_automaton_steps hands to the rule, with one thing wrong at a time
struct Block {
  int have_set = 1, have_g = 1, have_frames = 1, have_xy = 1, xy_per_step = 0, n_steps = 2, n = 2, input_size = 7,
      output_size = 3, bottom = 0;
  int width = 5, height = 4, len_y = 1, len_c = 2, len_pos = 2, edges = 1;
  int oy[2] = {0, 0}, oc[4] = {1, 0, 0, -1};
  int xy[8] = {0, 0, 4, 3, 1, 1, 2, 2};
  bool null_y = false, null_c = false;
};
static void refusal_line(const char *name, const Block &b) {
  const AutomatonRule g = {b.width, b.height, b.null_y ? nullptr : b.oy, b.len_y, b.null_c ? nullptr : b.oc, b.len_c, b.len_pos,
                           b.edges};
  const int code = automaton_block_refusal(b.have_set, b.have_g ? &g : nullptr, b.have_frames, b.have_xy ? b.xy : nullptr,
                                           b.xy_per_step, b.n_steps, b.n, b.input_size, b.output_size, b.bottom);
  printf("%s=%d %s\n", name, code, automaton_block_refusal_text(code));
}

int main(int argc, char **argv) {
  const char *mode = argc > 1 ? argv[1] : "";
  if (!strcmp(mode, "block") && argc == 12) {
    const int w = atoi(argv[2]), h = atoi(argv[3]), edges = atoi(argv[4]), len_pos = atoi(argv[5]);
    const int T = atoi(argv[7]), n = atoi(argv[8]), per_step = atoi(argv[9]);
    const int room = 8 * (int)strlen(argv[6]) + 1;
    std::vector<int> oy(2 * room), oc(2 * room);
    int ny = 0, nc = 0;
    if (automaton_parse_offsets(argv[6], oy.data(), &ny, oc.data(), &nc, room)) {
      return 3;
    }
    const std::vector<unsigned char> film = read_file(argv[10]);
    const std::vector<unsigned char> raw = read_file(argv[11]);
    std::vector<int> xy(raw.size() / sizeof(int));
    memcpy(xy.data(), raw.data(), xy.size() * sizeof(int));
    if (film.size() != (size_t)(T + 1) * 3 * w * h || xy.size() != (size_t)(per_step ? T : 1) * n * 2) {
      fprintf(stderr, "%zu bytes of film and %zu integers of positions are not this block's\n", film.size(), xy.size());
      return 2;
    }
    const AutomatonRule g = {w, h, oy.data(), ny, oc.data(), nc, len_pos, edges};
    if (automaton_block_refusal(1, &g, 1, xy.data(), per_step, T, n, automaton_input_size(&g), 3, 0)) {
      return 4;
    }
    for (int t = 0; t < T; t++)
      for (int j = 0; j < n; j++) {
        const int *p = automaton_train_xy(xy.data(), per_step, n, t, j);
        for (int i = 0; i < automaton_input_size(&g); i++) print_bits(automaton_train_input(g, film.data(), t, p[0], p[1], i));
      }
    for (int t = 0; t < T; t++)
      for (int j = 0; j < n; j++) {
        const int *p = automaton_train_xy(xy.data(), per_step, n, t, j);
        for (int k = 0; k < 3; k++) print_bits(automaton_train_target(g, film.data(), t, p[0], p[1], k));
      }
    printf("\n");
    return 0;
  }
  if (!strcmp(mode, "momentum") && argc == 5) {
    print_bits(automaton_train_momentum((unsigned)strtoul(argv[2], nullptr, 10), strtof(argv[3], nullptr), strtof(argv[4], nullptr)));
    printf("\n");
    return 0;
  }
  if (!strcmp(mode, "refusals") && argc == 2) {
    Block b;
    refusal_line("valid", b);
    b = Block(); b.xy_per_step = 1; refusal_line("valid per step", b);
    b = Block(); b.edges = 0; refusal_line("valid wrapped", b);
    b = Block(); b.len_c = 0; b.null_c = true; b.input_size = 3; refusal_line("valid empty C", b);
    b = Block(); b.have_set = 0; refusal_line("no set", b);
    b = Block(); b.have_g = 0; refusal_line("no geometry", b);
    b = Block(); b.have_frames = 0; refusal_line("no frames", b);
    b = Block(); b.have_xy = 0; refusal_line("no xy", b);
    b = Block(); b.n_steps = 0; refusal_line("no steps", b);
    b = Block(); b.n_steps = -3; refusal_line("negative steps", b);
    b = Block(); b.width = 0; refusal_line("width 0", b);
    b = Block(); b.height = -1; refusal_line("height -1", b);
    b = Block(); b.width = 1 << 16; b.height = 1 << 15; refusal_line("2^31 cells", b);
    b = Block(); b.len_y = -1; refusal_line("len_y -1", b);
    b = Block(); b.len_c = -1; refusal_line("len_c -1", b);
    b = Block(); b.null_y = true; refusal_line("NULL Y list", b);
    b = Block(); b.null_c = true; refusal_line("NULL C list", b);
    b = Block(); b.len_pos = 1; refusal_line("len_pos 1", b);
    b = Block(); b.len_pos = 4; refusal_line("len_pos 4", b);
    b = Block(); b.input_size = 8; refusal_line("an input too many", b);
    b = Block(); b.len_pos = 3; refusal_line("an input too few", b);
    b = Block(); b.output_size = 2; refusal_line("two outputs", b);
    b = Block(); b.bottom = 1; refusal_line("bottom layer", b);
    b = Block(); b.edges = 0; b.oc[3] = -4; refusal_line("wrap as long as the grid", b);
    b = Block(); b.oc[3] = -4; refusal_line("valid clamped long offset", b);
    b = Block(); b.n = 0; refusal_line("no trainers", b);
    b = Block(); b.xy[2] = 5; refusal_line("x is width", b);
    b = Block(); b.xy[3] = 4; refusal_line("y is height", b);
    b = Block(); b.xy[0] = -1; refusal_line("x -1", b);
    b = Block(); b.xy[1] = -1; refusal_line("y -1", b);
    b = Block(); b.xy[6] = 9; refusal_line("valid: outside behind the one list", b);
    b = Block(); b.xy_per_step = 1; b.xy[6] = 9; refusal_line("outside in the second step's list", b);
    return 0;
  }
  fprintf(stderr, "see the head of tests/automaton_train_rule_harness.cpp\n");
  return 2;
}
