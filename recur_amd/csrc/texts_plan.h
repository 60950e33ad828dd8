/* texts_plan.h -- how a batch of texts of different lengths is laid over state rows for rnn_amd_run_texts: the order, the
 * waves and the row counts, apart from the launches.
 *
 * texts_plan_make() reads lens, skips, n_texts and a wave width W and makes no HIP call, so the host compiler alone builds
 * it and tests/test_texts_plan.py asks it on a machine without a GPU.  Texts shorter than 2 symbols have nothing to score
 * and take no row.  The rest are ordered longest first (stable: equal lengths keep the caller's order) and cut into waves
 * of W rows.  A wave runs for `steps` = its longest text's len - 1 forward passes, and at step t the texts that still
 * have a symbol to feed, len - 1 > t, are -- because of the order -- the wave's first texts_plan_active() rows: the host
 * shrinks nrows launch by launch and no kernel needs a liveness mask.  `order` maps a plan row back to the caller's
 * index.  Plain C (and valid C++). */
#ifndef RAMD_TEXTS_PLAN_H
#define RAMD_TEXTS_PLAN_H 1
#include <stdlib.h>

#define TEXTS_PLAN_WIDTH 256 /* the row count the forward GEMM is tuned at */

typedef struct TextsWave {
  int row0, nrows; /* plan rows [row0, row0 + nrows) */
  int steps;       /* forward passes: the longest text's len - 1 */
} TextsWave;

typedef struct TextsPlan {
  int n_rows;  /* texts that take a row */
  int *order;  /* [n_rows] plan row -> the caller's index */
  int *len;    /* [n_rows] lens and skips in plan order */
  int *skip;
  int n_waves;
  TextsWave *waves;
} TextsPlan;

/* sort key of a text: the longer first, the caller's index among equals */
static inline int texts_plan_cmp(const void *a, const void *b) {
  const long long x = *(const long long *)a, y = *(const long long *)b;
  return x < y ? -1 : (x > y);
}

static inline void texts_plan_free(TextsPlan *p) {
  free(p->order);
  free(p->len);
  free(p->skip);
  free(p->waves);
  p->order = p->len = p->skip = NULL;
  p->waves = NULL;
  p->n_rows = p->n_waves = 0;
}

/* skips == NULL: all zeros; width < 1: TEXTS_PLAN_WIDTH.  Returns 0, or -1 when memory runs out (nothing to free). */
static inline int texts_plan_make(TextsPlan *p, const int *lens, const int *skips, int n_texts, int width) {
  p->n_rows = p->n_waves = 0;
  p->order = p->len = p->skip = NULL;
  p->waves = NULL;
  if (width < 1) {
    width = TEXTS_PLAN_WIDTH;
  }
  int n = 0;
  for (int k = 0; k < n_texts; k++) {
    n += lens[k] >= 2;
  }
  if (n == 0) {
    return 0;
  }
  const int n_waves = (n + width - 1) / width;
  long long *keys = (long long *)malloc((size_t)n * sizeof(long long));
  p->order = (int *)malloc((size_t)n * sizeof(int));
  p->len = (int *)malloc((size_t)n * sizeof(int));
  p->skip = (int *)malloc((size_t)n * sizeof(int));
  p->waves = (TextsWave *)malloc((size_t)n_waves * sizeof(TextsWave));
  if (!keys || !p->order || !p->len || !p->skip || !p->waves) {
    free(keys);
    texts_plan_free(p);
    return -1;
  }
  n = 0;
  for (int k = 0; k < n_texts; k++) {
    if (lens[k] >= 2) {
      keys[n++] = ((long long)(0x7fffffff - lens[k]) << 32) | (long long)k;
    }
  }
  qsort(keys, (size_t)n, sizeof(long long), texts_plan_cmp);
  for (int r = 0; r < n; r++) {
    const int k = (int)(keys[r] & 0x7fffffff);
    p->order[r] = k;
    p->len[r] = lens[k];
    p->skip[r] = skips ? skips[k] : 0;
  }
  free(keys);
  for (int w = 0; w < n_waves; w++) {
    p->waves[w].row0 = w * width;
    p->waves[w].nrows = (n - w * width < width) ? n - w * width : width;
    p->waves[w].steps = p->len[w * width] - 1;
  }
  p->n_rows = n;
  p->n_waves = n_waves;
  return 0;
}

/* a(t): the rows of wave w that feed a symbol at step t -- its texts with len - 1 > t, a prefix of the wave.  Non-increasing
 * in t, at least 1 for t < steps, 0 from there on. */
static inline int texts_plan_active(const TextsPlan *p, int w, int t) {
  const int *len = p->len + p->waves[w].row0;
  int lo = 0, hi = p->waves[w].nrows; /* the first row with len - 1 <= t (lengths descend) */
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (len[mid] - 1 > t) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  return lo;
}

/* where each row of wave w keeps its per-step values when every step of every row leaves per_step of them (the trace of
 * rnn_amd_trace_texts): off[j], for the wave's nrows rows, is the prefix sum of (len - 1) * per_step in plan order.
 * Returns the wave's total.  Lengths descend through the plan, so wave 0's total is the largest. */
static inline unsigned long long texts_plan_trace_offsets(const TextsPlan *p, int w, int per_step, unsigned long long *off) {
  const int *len = p->len + p->waves[w].row0;
  unsigned long long at = 0;
  for (int j = 0; j < p->waves[w].nrows; j++) {
    off[j] = at;
    at += (unsigned long long)(len[j] - 1) * (unsigned long long)per_step;
  }
  return at;
}

#endif
