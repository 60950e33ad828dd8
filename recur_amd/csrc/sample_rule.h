/* sample_rule.h -- how the next symbol of a text is drawn from a row of scores, stated once: for k_texts_continue
 * (kernels_rows.hip), which runs it with one wave per row, and for any host compiler alone (tests/sample_rule_harness.cpp
 * runs it under g++ against the oracle).  No HIP header is needed: under hipcc the functions are host and device
 * functions, elsewhere plain inline ones.
 *
 * The arithmetic is the reference's, as char_sampling.c restates it for the host (badmaths.h:71-156,
 * charmodel-predict.c:29-60), operation for operation, because a sampler is discontinuous -- one probability that rounds
 * the other way moves one draw, and every symbol after it:
 *   clamped softmax   shift the scores so that the largest is <= 50 and, where that leaves room, the smallest >= -60;
 *                     exp(score + shift) with the caller's fast exponential; the total in index order, in float; every
 *                     element DIVIDED by the total
 *   bias              bias != 0: p[i] = p[i] * bias + score[i], a multiplication and then an addition (never fused), and
 *                     the clamped softmax of that
 *   greedy pick       bias >= SAMPLE_GREEDY_BIAS: no draw, the LAST of equal maxima of the scores
 *   draw              u = (float)rand_double, rand_double being 52 bits of one rand64 under the exponent of 1.0, minus
 *                     1.0; the pick is the first i whose running total of p (float, index order) exceeds u; a u beyond
 *                     the rounded total draws again, one rand64 per attempt
 *   attempt cap       SAMPLE_MAX_ATTEMPTS attempts without a pick (a total that is NaN never yields one) end with
 *                     SAMPLE_FAILED instead of another attempt: with real probabilities the total is within rounding of
 *                     1 and the cap is never met, and device code must not loop on data
 *
 * Who does the work is an argument, a "team": its members share the strided loops, agree on the extremes and fence their
 * writes to p from one another's reads.  SampleSolo is a team of one (the host; a single lane); the kernel's team is a
 * wave.  The exponential and the generator are arguments too: the kernel passes fast_expf_dev and dev_rand64, a host
 * caller whatever it has.  A GCC caller compiles with -ffp-contract=off (clang takes the pragma below). */
#ifndef RAMD_SAMPLE_RULE_H
#define RAMD_SAMPLE_RULE_H 1

#if defined(__HIP__) || defined(__HIPCC__)
#define RAMD_HD __attribute__((host)) __attribute__((device)) inline
#else
#define RAMD_HD inline
#endif
#if defined(__clang__)
#define RAMD_FP_UNFUSED _Pragma("clang fp contract(off)")
#else
#define RAMD_FP_UNFUSED
#endif

#define SAMPLE_MAX_ATTEMPTS 64
#define SAMPLE_FAILED (-1)
#define SAMPLE_GREEDY_BIAS 100.0f

/* a team of one */
struct SampleSolo {
  RAMD_HD int lane() const { return 0; }
  RAMD_HD int stride() const { return 1; }
  RAMD_HD void extremes(float &, float &) const {} /* the members' (lo, hi) into the team's, in every member */
  RAMD_HD void fence() const {}                    /* the members' writes to p are visible to all of them */
};

/* badmaths.h:71-111: the shift that brings a row into the exponential's domain, from its smallest and largest value */
RAMD_HD float sample_shift(float lo, float hi) {
  RAMD_FP_UNFUSED
  if (hi > 50.0f) {
    return 50.0f - hi;
  }
  if (lo < -60.0f) {
    const float up = -60.0f - lo, room = 50.0f - hi;
    return up < room ? up : room;
  }
  return 0.0f;
}

/* dst = exp(src + shift) / their total.  dst may be src.  An argument that is not finite (an infinite score) becomes NaN
 * without entering the exponential, whose range reduction would not end on it: the row then has no total and the draw
 * fails at the cap. */
template <class EXP, class TEAM>
RAMD_HD void sample_softmax(float *dst, const float *src, int n, EXP fast_exp, const TEAM &team) {
  RAMD_FP_UNFUSED
  float lo = src[0], hi = src[0];
  for (int i = team.lane(); i < n; i += team.stride()) {
    hi = src[i] > hi ? src[i] : hi;
    lo = src[i] < lo ? src[i] : lo;
  }
  team.extremes(lo, hi);
  const float shift = sample_shift(lo, hi);
  for (int i = team.lane(); i < n; i += team.stride()) {
    const float x = src[i] + shift;
    dst[i] = __builtin_fabsf(x) <= 3.0e38f ? fast_exp(x) : __builtin_nanf("");
  }
  team.fence();
  float total = 0.0f; /* every member adds up the whole row, in index order: the same value in all of them */
  for (int i = 0; i < n; i++) {
    total += dst[i];
  }
  team.fence();
  for (int i = team.lane(); i < n; i += team.stride()) {
    dst[i] = dst[i] / total;
  }
  team.fence();
}

/* the distribution the draw is made from (badmaths.h:143-156); p and score are different arrays of n floats */
template <class EXP, class TEAM>
RAMD_HD void sample_distribution(float *p, const float *score, int n, float bias, EXP fast_exp, const TEAM &team) {
  RAMD_FP_UNFUSED
  sample_softmax(p, score, n, fast_exp, team);
  if (bias != 0) {
    for (int i = team.lane(); i < n; i += team.stride()) {
      const float scaled = p[i] * bias;
      p[i] = scaled + score[i];
    }
    team.fence();
    sample_softmax(p, p, n, fast_exp, team);
  }
}

/* bias >= SAMPLE_GREEDY_BIAS: the last of equal maxima, as the reference's >= picks (one member's work) */
RAMD_HD int sample_greedy(const float *score, int n) {
  int best = 0;
  for (int i = 1; i < n; i++) {
    if (score[i] >= score[best]) {
      best = i;
    }
  }
  return best;
}

/* recur-rng.h:57-78, then the sampler's conversion to float (charmodel-predict.c:45) */
RAMD_HD float sample_uniform(unsigned long long r64) {
  unsigned long long bits = (r64 & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull;
  double d;
  __builtin_memcpy(&d, &bits, sizeof d);
  return (float)(d - 1.0);
}

/* the first i whose running total of p exceeds u, or SAMPLE_FAILED when none does */
RAMD_HD int sample_pick(const float *p, int n, float u) {
  RAMD_FP_UNFUSED
  float reached = 0.0f;
  for (int i = 0; i < n; i++) {
    reached += p[i];
    if (u < reached) {
      return i;
    }
  }
  return SAMPLE_FAILED;
}

/* draws until a u falls under the total, SAMPLE_MAX_ATTEMPTS times at the most; rand64() is one step of the row's
 * generator (one member's work) */
template <class RAND64>
RAMD_HD int sample_draw(const float *p, int n, RAND64 &rand64) {
  for (int attempt = 0; attempt < SAMPLE_MAX_ATTEMPTS; attempt++) {
    const int pick = sample_pick(p, n, sample_uniform(rand64()));
    if (pick != SAMPLE_FAILED) {
      return pick;
    }
  }
  return SAMPLE_FAILED;
}

#endif
