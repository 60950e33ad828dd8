/* dream_rule.h -- how parrot's player turns a net's answer into its own next input, stated once: for k_dream_step
 * (kernels_rows.hip), which runs it with one workgroup per sequence, for dream_api.c and for any host compiler alone
 * (tests/dream_rule_harness.cpp runs it under g++ against numpy and the oracle).  No HIP header is needed: under hipcc the
 * functions are host and device functions, elsewhere plain inline ones.  dream_draw takes the generator as an argument,
 * as sample_rule.h's draw does, and is C++; the rest is C.
 *
 * The arithmetic is the reference's, operation for operation, because the loop is closed: a frame that rounds the other
 * way is the next frame's input, and every frame behind it moves.
 *   dream_tanh   (fast_tanhf, badmaths.h:55-68; tanh_opinion, gstparrot.c:566) x <= -4.97f is -1.0f and x >= 4.97f is
 *                1.0f; otherwise Lambert's continued fraction, with x2 = x * x:
 *                    a = x * (135135 + x2 * (17325 + x2 * (378 + x2)))
 *                    b = 135135 + x2 * (62370 + x2 * (3150 + x2 * 28))
 *                and a / b, every operation one fp32 rounding in that order, none fused.  NaN fails both comparisons and
 *                stays NaN through the fraction; an infinity is clamped.
 *   dream_next   (gstparrot.c:576) a * (1.0f + noise * g), g being what cheap_gaussian_noise returns: the product
 *                noise * g, the sum and the last product are three roundings -- never a + a * g.  With noise == 1.0f the
 *                first product is exact and the value is the reference's answer[i] *= 1.0f + cheap_gaussian_noise(rng).
 *   draw order   one generator per sequence, one value per output in index order, frame after frame (dream_draw).  With
 *                noise == 0.0f nothing is drawn (dream_draws).
 * A GCC caller compiles with -ffp-contract=off (clang takes the pragma below). */
#ifndef RAMD_DREAM_RULE_H
#define RAMD_DREAM_RULE_H 1
#include <stddef.h>

#ifndef RAMD_HD
#if defined(__HIP__) || defined(__HIPCC__)
#define RAMD_HD __attribute__((host)) __attribute__((device)) inline
#elif defined(__cplusplus)
#define RAMD_HD inline
#else
#define RAMD_HD static inline
#endif
#endif
#ifndef RAMD_FP_UNFUSED
#if defined(__clang__)
#define RAMD_FP_UNFUSED _Pragma("clang fp contract(off)")
#else
#define RAMD_FP_UNFUSED
#endif
#endif

#define DREAM_TANH_EXTREME 4.97f

/* badmaths.h:55-68 */
RAMD_HD float dream_tanh(float x) {
  RAMD_FP_UNFUSED
  if (x <= -DREAM_TANH_EXTREME) {
    return -1.0f;
  }
  if (x >= DREAM_TANH_EXTREME) {
    return 1.0f;
  }
  const float x2 = x * x;
  const float a = x * (135135.0f + x2 * (17325.0f + x2 * (378.0f + x2)));
  const float b = 135135.0f + x2 * (62370.0f + x2 * (3150.0f + x2 * 28.0f));
  return a / b;
}

/* gstparrot.c:576, the noise scaled */
RAMD_HD float dream_next(float a, float noise, float g) {
  RAMD_FP_UNFUSED
  const float scaled = noise * g;
  const float gain = 1.0f + scaled;
  return a * gain;
}

/* whether a frame draws at all: noise == 0 leaves every generator alone */
RAMD_HD int dream_draws(float noise) { return noise != 0.0f; }

#ifdef __cplusplus
/* one frame's draws of one sequence: gz[i * stride] = gaussian() for i = 0 .. n - 1 in index order (one member's work:
 * the generator is a recurrence); gaussian() is one cheap_gaussian_noise of the sequence's generator */
template <class GAUSSIAN>
RAMD_HD void dream_draw(float *gz, int n, size_t stride, GAUSSIAN &gaussian) {
  for (int i = 0; i < n; i++) {
    gz[(size_t)i * stride] = gaussian();
  }
}
#endif

#endif
