/* classify_rule.h -- the per-row rule of rnn_amd_classify_texts (classify_texts_api.c, k_classify_step in
 * kernels_rows.hip) and the arithmetic that finishes its sums (rnn_amd_char_classify_texts), apart from the launches.
 *
 * A text of len symbols is fed whole: forward pass t, t = 0 .. len - 1, takes the one-hot of symbol t, and the output row it
 * leaves is symbol t's opinion (text-classify-results.c:83-122, charmodel-classify.c:174-196).  Three questions per
 * (text, t), each stated once here:
 *   fed      t < len: symbol t has a forward pass;
 *   scored   fed, and t >= skip: the softmax of that pass's output row is added to the text's sums and sums of squares
 *            (a skip below 0 is a skip of 0; a skip >= len feeds the text and scores nothing);
 *   counted  scored, and the symbol's class byte is not CLASSIFY_NO_CLASS (charmodel.h's NO_CLASS): the symbol is also held
 *            against its class in the text's RnnAmdClassScore.
 * The kernel asks the second halves only -- the plan's row order has answered `fed` for it (texts_plan.h: the rows that
 * still run are a prefix) -- so those stand on their own: classify_skip_passed and classify_has_class.
 * A class byte is valid when it is CLASSIFY_NO_CLASS or names an output: classify_class_ok.
 *
 * The finish (classify_finish): per text and class, from the sum and the sum of squares of a probability over n scored
 * symbols, in double:  mean = sum / n,  stddev = sqrt(max(0, sumsq / n - mean * mean)).  The clamp is deliberate: the
 * reference forms the difference in float without one and prints NaN where rounding takes it below zero.  n < 1 (nothing
 * was scored) gives zeros.  classify_scored_count is that n for one text: len - ignore_start, not below 0.
 *
 * No HIP: the host compiler alone builds it and tests/test_classify_rule.py asks it on a machine without a GPU.  Plain C
 * (and valid C++, host and device). */
#ifndef RAMD_CLASSIFY_RULE_H
#define RAMD_CLASSIFY_RULE_H 1
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CLASSIFY_RULE_FN __host__ __device__ static inline
#else
#define CLASSIFY_RULE_FN static inline
#endif

#define CLASSIFY_NO_CLASS 0xFF

CLASSIFY_RULE_FN int classify_fed(int len, int t) { return t >= 0 && t < len; }
CLASSIFY_RULE_FN int classify_skip_passed(int skip, int t) { return t >= skip; }
CLASSIFY_RULE_FN int classify_has_class(int class_byte) { return class_byte != CLASSIFY_NO_CLASS; }

CLASSIFY_RULE_FN int classify_scored(int len, int skip, int t) { return classify_fed(len, t) && classify_skip_passed(skip, t); }
CLASSIFY_RULE_FN int classify_counted(int len, int skip, int t, int class_byte) {
  return classify_scored(len, skip, t) && classify_has_class(class_byte);
}
CLASSIFY_RULE_FN int classify_class_ok(int class_byte, int output_size) {
  return class_byte == CLASSIFY_NO_CLASS || (class_byte >= 0 && class_byte < output_size);
}

/* how many symbols of a text of len are scored behind ignore_start of them */
CLASSIFY_RULE_FN int classify_scored_count(int len, int ignore_start) {
  const int skip = ignore_start > 0 ? ignore_start : 0;
  return len > skip ? len - skip : 0;
}
CLASSIFY_RULE_FN void classify_finish(double sum, double sumsq, int n, double *mean, double *stddev) {
  if (n < 1) {
    *mean = *stddev = 0.0;
    return;
  }
  const double m = sum / n;
  const double var = sumsq / n - m * m;
  *mean = m;
  *stddev = var > 0.0 ? sqrt(var) : 0.0;
}

#endif
