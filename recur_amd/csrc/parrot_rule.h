/* parrot_rule.h -- the loss of parrot's trainer (train_net, gstparrot.c:464-477), stated once: for
 * k_dense_loss_row<TanhLossRule> and k_text_top<3> (kernels_loss.hip) and for any host compiler alone
 * (tests/parrot_rule_harness.cpp runs it under g++
 * against numpy).  No HIP header is needed: under hipcc the functions are host and device functions, elsewhere plain
 * inline ones.  The answer itself is dream_rule.h's dream_tanh (fast_tanhf), which the player uses too.
 *
 *   parrot_error  (gstparrot.c:473) with a = dream_tanh(output):
 *                     slope = 1.0f - a * a
 *                     diff  = target - a
 *                 and slope * diff: four fp32 roundings in that order (the square, the slope, the difference, the
 *                 product), none fused -- never diff - a * a * diff, never fmaf(-a, a, 1.0f).
 *   parrot_loss   diff * diff, the term the set's statistics add up per output (the plugin has no such figure; a
 *                 trainer that stays on the device needs one that does not visit the host).
 *
 * OUTPUTS THAT ARE NOT FINITE follow dream_tanh: an infinite output is clamped to +-1.0f, so its slope is exactly 0 and
 * its error exactly 0 for every finite target; a NaN output gives a NaN answer and a NaN error.  Both are elementwise.
 * (The sigmoid's rule differs: there an infinity is NaN, fast_exp_rule.h.)
 * A GCC caller compiles with -ffp-contract=off (clang takes the pragma below). */
#ifndef RAMD_PARROT_RULE_H
#define RAMD_PARROT_RULE_H 1
#include "dream_rule.h"

/* gstparrot.c:473; a is the answer, fast_tanhf of the output */
RAMD_HD float parrot_error(float a, float target) {
  RAMD_FP_UNFUSED
  const float sq = a * a;
  const float slope = 1.0f - sq;
  const float diff = target - a;
  return slope * diff;
}

/* one output's term of the progress figure */
RAMD_HD float parrot_loss(float a, float target) {
  RAMD_FP_UNFUSED
  const float diff = target - a;
  return diff * diff;
}

/* Which blocks of frames rnn_amd_set_dense_steps_tanh takes -- frames [n_steps + 1][n_nets][ld], every frame an input row
 * of input_size floats and a target row of n -- stated here so that it is asked without a device (the call itself prints
 * the refusal and aborts, as the set API does): 0, or the first thing that is wrong. */
enum {
  PARROT_BLOCK_OK = 0,
  PARROT_BLOCK_NO_FRAMES = 1, /* NULL frames */
  PARROT_BLOCK_NO_STEPS = 2,  /* n_steps < 1: a generation needs two frames */
  PARROT_BLOCK_TARGETS = 3,   /* n < 1 or n > output_size */
  PARROT_BLOCK_LD = 4         /* ld < input_size or ld < n: a row does not hold a frame */
};
RAMD_HD int parrot_block_refusal(int have_frames, int n_steps, int ld, int input_size, int n, int output_size) {
  if (!have_frames) {
    return PARROT_BLOCK_NO_FRAMES;
  }
  if (n_steps < 1) {
    return PARROT_BLOCK_NO_STEPS;
  }
  if (n < 1 || n > output_size) {
    return PARROT_BLOCK_TARGETS;
  }
  if (ld < input_size || ld < n) {
    return PARROT_BLOCK_LD;
  }
  return PARROT_BLOCK_OK;
}
RAMD_HD const char *parrot_block_refusal_text(int refusal) {
  switch (refusal) {
  case PARROT_BLOCK_OK: return "a block it takes";
  case PARROT_BLOCK_NO_FRAMES: return "no frames";
  case PARROT_BLOCK_NO_STEPS: return "fewer than one generation";
  case PARROT_BLOCK_TARGETS: return "targets outside the outputs";
  case PARROT_BLOCK_LD: return "rows too short for a frame";
  }
  return "?";
}

#endif
