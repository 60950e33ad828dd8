// kernels_automaton_train.hip -- the one gather launch of rnn_amd_set_automaton_steps (automaton_train_api.c): every
// trainer's dense input row and target row of every generation of a block, from the bytes of the block's film on the
// device, by automaton_train_rule.h's statement of fill_net_inputs and train_net (gstrnnca.c:669-708).  It stands apart
// from kernels_rows.hip because it writes no state row: its rows are a training set's dense inputs, which the forward pass
// reads as it reads the staged rows of rnn_amd_set_opinion.
#include "k_common.h"
#include "automaton_train_rule.h"
#pragma clang fp contract(off)

// RamdAutomatonTrainRows's launch.  The floats to write are numbered once -- the rows [n_steps][n][input_size], then the
// targets [n_steps][n][3] -- and a grid-stride loop of 256-thread workgroups walks the numbers: consecutive threads write
// consecutive floats, so the stores are coalesced, and every float has one writer (no atomics, no memset).  The bytes are
// scattered reads of a film of a few hundred KB, which stays in L2.  The position inputs are automaton_position's, the
// third evaluated in double; the file compiles unfused, as the rule's pragma asks.
__global__ __launch_bounds__(256) void k_automaton_train_rows(RamdAutomatonTrainRows p) {
  const long long n_rows = (long long)p.n_steps * p.n;
  const long long row_floats = n_rows * p.input_size, all = row_floats + 3 * n_rows;
  const long long stride = (long long)gridDim.x * 256;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < all; q += stride) {
    const bool is_target = q >= row_floats;
    const long long at = is_target ? q - row_floats : q;
    const int width = is_target ? 3 : p.input_size;
    const long long row = at / width;
    const int i = (int)(at - row * width);
    const int t = (int)(row / p.n), j = (int)(row - (long long)t * p.n);
    const int *xy = automaton_train_xy(p.xy, p.xy_per_step, p.n, t, j);
    const int x = xy[0], y = xy[1];
    if (is_target) {
      p.targets[at] = automaton_train_target(p.g, p.frames, t, x, y, i);
    } else {
      p.rows[at] = automaton_train_input(p.g, p.frames, t, x, y, i);
    }
  }
}

#pragma clang fp contract(fast)

extern "C" void ramd_launch_automaton_train_rows(ramd_stream_t st, const RamdAutomatonTrainRows *p) {
  const AutomatonRule *g = &p->g;
  if (!p->frames || !p->xy || !p->rows || !p->targets || p->n_steps < 1 || p->n < 1 || g->width < 1 || g->height < 1 ||
      g->len_y < 0 || g->len_c < 0 || (g->len_y > 0 && !g->offsets_y) || (g->len_c > 0 && !g->offsets_c) ||
      (g->len_pos != 2 && g->len_pos != 3) || automaton_input_size(g) != p->input_size) {
    fprintf(stderr, "librecur_amd: ramd_launch_automaton_train_rows: %d generations of %d trainers, %d + 2 * %d + %d inputs "
                    "for rows of %d\n", p->n_steps, p->n, g->len_y, g->len_c, g->len_pos, p->input_size);
    abort();
  }
  const long long all = (long long)p->n_steps * p->n * (p->input_size + 3);
  const long long blocks = (all + 255) / 256;
  /* (a grid-stride loop: 8 workgroups per compute unit's worth is all the launch ever needs) */
  RAMD_LAUNCH(k_automaton_train_rows, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, (hipStream_t)st, *p);
}
