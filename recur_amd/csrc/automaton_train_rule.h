/* automaton_train_rule.h -- what rnnca's trainers are fed and scored against (gstrnnca.c: fill_net_inputs 669-691, train_net
 * 693-716, maybe_learn 718-750), stated once on top of automaton_rule.h: for k_automaton_train_rows
 * (kernels_automaton_train.hip), which runs it for every trainer and every generation of a block in one launch, for
 * automaton_train_api.c (gnu11 C: the refusals, the momentum) and for any host compiler alone
 * (tests/automaton_train_rule_harness.cpp runs it under g++ against numpy).  No HIP header is needed.
 *
 * A block is a film of n_steps + 1 frames of bytes, frames[n_steps + 1][3][cells], and the trainers' positions
 * xy[n_steps or 1][n][2] as (x, y).  Of generation t, for the trainer at (x, y):
 *   input i      automaton_input(g, x, y, i, level) with level(plane, cell) the byte frames[t][plane][cell]: the player's
 *                rule, every rounding of it, with the grid's `edges` as it is given.  (The plugin always trains with
 *                clamped edges, gstrnnca.c:698: a caller that wants the plugin passes edges = 1.)
 *   target k     (k = 0, 1, 2: Y, Cb, Cr; gstrnnca.c:702-708) automaton_unit(frames[t + 1][k][y * width + x]): the byte
 *                times the rounded reciprocal of 255, of the frame AFTER, at the trainer's own cell
 *   momentum     (gstrnnca.c:726-728) with momentum_soft_start == 0 the momentum as it is; otherwise
 *                rnn_calculate_momentum_soft_start(generation, momentum, momentum_soft_start) =
 *                min(momentum, 1 - s / (1 + generation + 2 s)) in float, of the net's generation in front of the update
 * and which blocks the call takes (automaton_block_refusal), asked without a device.
 * A GCC caller of the input rule compiles with -ffp-contract=off (clang takes the pragma). */
#ifndef RAMD_AUTOMATON_TRAIN_RULE_H
#define RAMD_AUTOMATON_TRAIN_RULE_H 1
#include <stddef.h>
#include "automaton_rule.h"

#ifndef RAMD_HD_MEMBER /* a member function of a functor both sides call */
#if defined(__HIP__) || defined(__HIPCC__)
#define RAMD_HD_MEMBER __attribute__((host)) __attribute__((device))
#else
#define RAMD_HD_MEMBER
#endif
#endif

/* The one gather launch of rnn_amd_set_automaton_steps (k_automaton_train_rows; the launcher is declared in
 * ramd_internal.h): for every generation t < n_steps and every trainer j < n the dense input row
 * rows[(t * n + j) * input_size + i] and the target row targets[(t * n + j) * 3 + k], by the rule above, from the block's
 * film.  g's offset lists are device arrays; with edges == 0 the caller has refused offsets the single wrap does not
 * bring back, and every (x, y) of xy lies inside the grid (automaton_block_refusal: checked on the host before the
 * launch).  Every float has one writer: no atomics, no memset.  All pointers are device pointers. */
typedef struct RamdAutomatonTrainRows {
  AutomatonRule g;             /* the grid                                                            */
  const unsigned char *frames; /* [n_steps + 1][3][cells] the block's film                            */
  const int *xy;               /* [xy_per_step ? n_steps : 1][n][2] (x, y) of every trainer           */
  int xy_per_step;             /* non-zero: a position list per generation                            */
  int n_steps, n;              /* generations, trainers                                               */
  int input_size;              /* len_y + 2 * len_c + len_pos: the floats of a row                    */
  float *rows;                 /* [n_steps][n][input_size] out                                        */
  float *targets;              /* [n_steps][n][3] out                                                 */
} RamdAutomatonTrainRows;

/* where generation t's position of trainer j lies in xy */
RAMD_HD const int *automaton_train_xy(const int *xy, int xy_per_step, int n, int t, int j) {
  return xy + 2 * ((size_t)(xy_per_step ? t : 0) * n + j);
}

/* gstrnnca.c:726-728 (recur-nn.c: rnn_calculate_momentum_soft_start) */
RAMD_HD float automaton_train_momentum(unsigned generation, float momentum, float momentum_soft_start) {
  RAMD_FP_UNFUSED
  if (momentum_soft_start == 0.0f) {
    return momentum;
  }
  const float x = momentum_soft_start;
  const float soft = 1.0f - x / (1.0f + (float)generation + 2.0f * x);
  return momentum < soft ? momentum : soft;
}

/* Which blocks rnn_amd_set_automaton_steps takes: 0, or the first thing that is wrong (the call prints the text and
 * aborts, as the set API does).  The grid's part is what rnn_amd_run_automaton refuses. */
enum {
  AUTOMATON_BLOCK_OK = 0,
  AUTOMATON_BLOCK_NULL = 1,     /* a NULL set, geometry, film or position list */
  AUTOMATON_BLOCK_NO_STEPS = 2, /* n_steps < 1: a generation needs two frames */
  AUTOMATON_BLOCK_GRID = 3,     /* width or height < 1, or more than INT_MAX cells */
  AUTOMATON_BLOCK_LISTS = 4,    /* a negative list length, or a NULL list that has pairs */
  AUTOMATON_BLOCK_LEN_POS = 5,  /* neither 2 nor 3 position inputs */
  AUTOMATON_BLOCK_INPUTS = 6,   /* input_size != len_y + 2 * len_c + len_pos */
  AUTOMATON_BLOCK_OUTPUTS = 7,  /* fewer than three outputs */
  AUTOMATON_BLOCK_BOTTOM = 8,   /* a set with a bottom layer */
  AUTOMATON_BLOCK_WRAP = 9,     /* a wrapped grid and an offset as long as it */
  AUTOMATON_BLOCK_TRAINERS = 10, /* no trainers */
  AUTOMATON_BLOCK_XY = 11       /* a trainer outside the grid */
};
RAMD_HD int automaton_block_refusal(int have_set, const AutomatonRule *g, int have_frames, const int *xy, int xy_per_step,
                                    int n_steps, int n, int input_size, int output_size, int bottom_layer) {
  if (!have_set || !g || !have_frames || !xy) {
    return AUTOMATON_BLOCK_NULL;
  }
  if (n_steps < 1) {
    return AUTOMATON_BLOCK_NO_STEPS;
  }
  if (g->width < 1 || g->height < 1 || g->width > 0x7fffffff / g->height) {
    return AUTOMATON_BLOCK_GRID;
  }
  if (g->len_y < 0 || g->len_c < 0 || (g->len_y > 0 && !g->offsets_y) || (g->len_c > 0 && !g->offsets_c)) {
    return AUTOMATON_BLOCK_LISTS;
  }
  if (g->len_pos != 2 && g->len_pos != 3) {
    return AUTOMATON_BLOCK_LEN_POS;
  }
  if ((long long)input_size != (long long)g->len_y + 2LL * g->len_c + g->len_pos) {
    return AUTOMATON_BLOCK_INPUTS;
  }
  if (output_size < 3) {
    return AUTOMATON_BLOCK_OUTPUTS;
  }
  if (bottom_layer) {
    return AUTOMATON_BLOCK_BOTTOM;
  }
  if (!g->edges) {
    for (int k = 0; k < g->len_y + g->len_c; k++) {
      const int *o = k < g->len_y ? g->offsets_y + 2 * k : g->offsets_c + 2 * (k - g->len_y);
      if (!automaton_wrap_reaches(o[0], o[1], g->width, g->height)) {
        return AUTOMATON_BLOCK_WRAP;
      }
    }
  }
  if (n < 1) {
    return AUTOMATON_BLOCK_TRAINERS;
  }
  const long long lists = xy_per_step ? n_steps : 1;
  for (long long q = 0; q < lists * n; q++) {
    const int x = xy[2 * q], y = xy[2 * q + 1];
    if (x < 0 || x >= g->width || y < 0 || y >= g->height) {
      return AUTOMATON_BLOCK_XY;
    }
  }
  return AUTOMATON_BLOCK_OK;
}
RAMD_HD const char *automaton_block_refusal_text(int refusal) {
  switch (refusal) {
  case AUTOMATON_BLOCK_OK: return "a block it takes";
  case AUTOMATON_BLOCK_NULL: return "a NULL set, geometry, film or position list";
  case AUTOMATON_BLOCK_NO_STEPS: return "fewer than one generation";
  case AUTOMATON_BLOCK_GRID: return "a grid without cells, or of too many";
  case AUTOMATON_BLOCK_LISTS: return "offset lists of negative length, or a NULL one";
  case AUTOMATON_BLOCK_LEN_POS: return "position inputs that are neither 2 nor 3";
  case AUTOMATON_BLOCK_INPUTS: return "a net whose inputs are not a cell's";
  case AUTOMATON_BLOCK_OUTPUTS: return "a net of fewer than three outputs";
  case AUTOMATON_BLOCK_BOTTOM: return "a set with a bottom layer";
  case AUTOMATON_BLOCK_WRAP: return "an offset the single wrap does not bring back";
  case AUTOMATON_BLOCK_TRAINERS: return "no trainers";
  case AUTOMATON_BLOCK_XY: return "a trainer outside the grid";
  }
  return "?";
}

#ifdef __cplusplus
struct AutomatonFilmLevels { /* frame t of the film is bytes in memory */
  const unsigned char *frame; /* frames + t * 3 * cells */
  int cells;
  RAMD_HD_MEMBER unsigned char operator()(int plane, int cell) const { return frame[(size_t)plane * cells + cell]; }
};

/* input i of generation t of the trainer at (x, y) */
RAMD_HD float automaton_train_input(const AutomatonRule &g, const unsigned char *frames, int t, int x, int y, int i) {
  const int cells = g.width * g.height;
  const AutomatonFilmLevels level = {frames + (size_t)t * 3 * cells, cells};
  return automaton_input(g, x, y, i, level);
}

/* target k of generation t of the trainer at (x, y): gstrnnca.c:702-708 */
RAMD_HD float automaton_train_target(const AutomatonRule &g, const unsigned char *frames, int t, int x, int y, int k) {
  const size_t cells = (size_t)g.width * g.height;
  return automaton_unit(frames[((size_t)(t + 1) * 3 + k) * cells + (size_t)y * g.width + x]);
}
#endif

#endif
