/* sigmoid_rule.h -- the loss of rnnca's trainer (train_net, gstrnnca.c:701-714), stated once: for k_sigmoid_mse_error,
 * k_dense_loss_row<SigmoidLossRule>, k_text_top<1> and k_sigmoid_outputs (kernels_loss.hip) and for any host compiler alone
 * (tests/sigmoid_rule_harness.cpp runs it under g++ against numpy and the oracle's fast_expf).  No HIP header is needed:
 * under hipcc the functions are host and device functions, elsewhere plain inline ones.  The exponential is the caller's
 * (a kernel passes fast_expf_dev, a host harness fast_exp_rule.h's fast_expf), as automaton_level takes it.
 *
 *   sigmoid_answer  fast_sigmoid (badmaths.h:31-44) of one output: 1.0f / (1.0f + fast_exp(-x * 1.0f)) -- the negation, the
 *                   product with the reference's steepness 1.0f, the exponential, the sum, the division, in that order
 *   sigmoid_error   (gstrnnca.c:710-712) with a the answer:
 *                       slope = a * (1.0f - a)
 *                       diff  = target - a
 *                   and slope * diff: four fp32 roundings in that order, none fused
 *   sigmoid_loss    diff * diff with the same diff, the term the set's statistics add up per output
 *
 * OUTPUTS THAT ARE NOT FINITE follow the exponential: fast_exp_rule.h's gives a NaN for either infinity, so the answer and
 * the error of an infinite output are NaN, as a NaN output's are (parrot's tanh clamps instead: parrot_rule.h).  This is
 * not automaton_level's sigmoid, which saturates: the player's bytes have no NaN to show.
 * A GCC caller compiles with -ffp-contract=off (clang takes the pragma below). */
#ifndef RAMD_SIGMOID_RULE_H
#define RAMD_SIGMOID_RULE_H 1
#include "fast_exp_rule.h"

/* badmaths.h:31-44 */
template <class EXP>
RAMD_HD float sigmoid_answer(float x, EXP fast_exp) {
  RAMD_FP_UNFUSED
  return 1.0f / (1.0f + fast_exp(-x * 1.0f));
}

/* gstrnnca.c:710-712; a is the answer */
RAMD_HD float sigmoid_error(float a, float target) {
  RAMD_FP_UNFUSED
  const float slope = a * (1.0f - a);
  const float diff = target - a;
  return slope * diff;
}

/* one output's term of the progress figure */
RAMD_HD float sigmoid_loss(float a, float target) {
  RAMD_FP_UNFUSED
  const float diff = target - a;
  return diff * diff;
}

#endif
