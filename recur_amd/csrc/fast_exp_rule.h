/* fast_exp_rule.h -- the reference's fast exponential (badmaths.h:14-29), stated once: for every loss and scoring kernel
 * (fast_expf_dev, k_top.h), for the host's ramd_fast_expf (rnn_init.c: the initialisers and char_sampling.c) and for any
 * host compiler alone (tests/fast_exp_rule_harness.cpp runs it under g++ against numpy, the oracle and the reference).  No
 * HIP header is needed: under hipcc the functions are host and device functions, elsewhere plain inline ones; it is C as
 * well as C++.
 *
 * The arithmetic is the reference's, operation for operation:
 *   scaling          while |x| > 0.2 (the comparison in double, as the C promotes it): x *= 0.125, one more round
 *   Pade (2, 2)      a = ((x + 3) * (x + 3) + 3) / ((x - 3) * (x - 3) + 3), every operation one fp32 rounding, none fused
 *   squaring back    three squarings per round
 * For every finite x -- up to FLT_MAX (44 rounds), the denormals and both zeros (none) -- the value and the number of
 * rounds are the reference's, bit for bit.
 *
 * What the reference does not have: its scaling loop does not end on an infinity (inf * 0.125 is inf).  Here an argument
 * that is not finite -- either infinity, any NaN -- gives a quiet NaN in no rounds, without entering the loop: this is the
 * only loop of the library's device code whose trip count is data's to decide, and it ends on every float.  A softmax with
 * an infinity or a NaN in it therefore has NaN exponentials, a NaN total and NaN likelihoods (include/recur_amd.h, "Rows
 * that are not finite").
 * A GCC caller compiles with -ffp-contract=off (clang takes the pragma below). */
#ifndef RAMD_FAST_EXP_RULE_H
#define RAMD_FAST_EXP_RULE_H 1

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

#define FAST_EXP_LARGEST_FINITE 3.40282346638528859811704183484516925e+38f /* FLT_MAX */

/* badmaths.h:14-29; *rounds is the number of scaling rounds made (for tests/fast_exp_rule_harness.cpp) */
RAMD_HD float fast_expf_rounds(float x, int *rounds) {
  RAMD_FP_UNFUSED
  int count = 0;
  *rounds = 0;
  if (!(__builtin_fabsf(x) <= FAST_EXP_LARGEST_FINITE)) {
    return __builtin_nanf(""); /* an infinity would never leave the loop below; a NaN would, and is a NaN already */
  }
  while (__builtin_fabsf(x) > 0.2) {
    x *= 0.125;
    count++;
  }
  *rounds = count;
  float a = ((x + 3) * (x + 3) + 3) / ((x - 3) * (x - 3) + 3);
  while (count) {
    a *= a;
    a *= a;
    a *= a;
    count--;
  }
  return a;
}

RAMD_HD float fast_expf(float x) {
  int rounds;
  return fast_expf_rounds(x, &rounds);
}

#endif
