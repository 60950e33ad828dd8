/* classify_train_rule.h -- what gstclassify's trainer decides per generation (maybe_learn, gstclassify.c:2180-2257, with
 * train_channel's loss 2070-2119 and the balanced-training draw 2096-2104, 2190-2215), stated once: for
 * rnn_amd_set_classify_steps (set_train.c), for rnn_amd_classify_generation and rnn_amd_classify_generations
 * (classify_host.c), for the gate the loss kernels write and k_apply reads (kernels_loss.hip, kernels_apply.hip) and for any
 * host compiler alone (tests/classify_train_rule_harness.cpp runs it under g++ against numpy).  No HIP header is needed.
 *
 * A block is features[n_steps][n][ld] and targets[n_steps][n][n_groups]; the outputs are n_groups class groups, group i
 * the columns group_offset[i] .. group_offset[i] + group_size[i] - 1.  Of generation t:
 *   trained    group i of stream j is trained iff 0 <= targets[t][j][i] < group_size[i]: any other value is "no label"
 *   active     stream j is active iff one of its groups is trained: its deltas are summed, its generation counter steps
 *              (recur-nn.c:765); a stream without a label keeps its error images and its counter
 *   no label   a generation without an active stream makes no delta call and no update (the forward pass, the ring advance
 *              and the conditioning still happen, as in maybe_learn)
 *   THE GATE   the reference updates `if (err_sum)`: err_sum is the float sum, in channel order, of every trained group's
 *              wrongness 1 - p[target].  Every term is >= 0 -- p is a softmax likelihood, e / sum with e one of sum's
 *              non-negative terms, so p <= 1 in float as well --, no term is -0 (1 - 1 is +0), and a sum of non-negative
 *              floats is zero iff every term is: no rounding brings a positive term back to zero, the sum only grows.  So
 *              `err_sum != 0` is "some trained stream's summed wrongness is not 0.0f", which is what a stream can decide
 *              alone (classify_gate_raises) and lane 0 of its loss kernel stores.  NaN raises the gate: if (err_sum) is
 *              true for NaN, and NaN != 0.0f.  The one way the two could differ is a p > 1 (a negative term that cancels a
 *              positive one): tests/test_classify_train_cases_cpu.py shows from the oracle's softmax that no likelihood
 *              exceeds 1 on the cases used.
 *              A closed gate leaves weights, momentum and aux arrays untouched; the delta arrays hold the generation's
 *              sums all the same, and the statistics the loop's figures.
 *   balanced   per generation the probability of using a labelled window of class c is
 *              powf(1 - seen[c] * (1 / (seen_total + 1)), bias), from the counts BEFORE the generation; then one draw per
 *              labelled (channel, group), channel-major, a float in [0, 1] from 64 bits of the prototype's generator.
 */
#ifndef RAMD_CLASSIFY_TRAIN_RULE_H
#define RAMD_CLASSIFY_TRAIN_RULE_H 1
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifndef RAMD_HD
#if defined(__HIP__) || defined(__HIPCC__)
#define RAMD_HD __attribute__((host)) __attribute__((device)) inline
#elif defined(__cplusplus)
#define RAMD_HD inline
#else
#define RAMD_HD static inline
#endif
#endif

/* a stream's summed wrongness raises the generation's gate iff it is not 0.0f (-0.0f is zero; NaN is not) */
RAMD_HD int classify_gate_raises(float wrong) { return wrong != 0.0f; }

/* is `target` a label of a group of `size` classes? */
RAMD_HD int classify_target_trains(int target, int size) { return target >= 0 && target < size; }

/* stream j of a generation is active iff one of its groups has a label; row: its n_groups targets */
RAMD_HD int classify_stream_active(const int *row, int n_groups, const int *group_size) {
  for (int i = 0; i < n_groups; i++) {
    if (classify_target_trains(row[i], group_size[i])) {
      return 1;
    }
  }
  return 0;
}

/* every generation's mask starts on a 4-byte boundary of the block's mask area */
RAMD_HD size_t classify_mask_stride(int n) { return ((size_t)n + 3) & ~(size_t)3; }

/* The host decisions of a block, from its targets: masks[t * classify_mask_stride(n) + j] = stream j is active at t (the
 * padding bytes are 0), active[t] = how many are (0: no delta call, no update), and generation[j] += 1 per generation in
 * which stream j is active (generation may be NULL).  Returns the number of trained groups of the block. */
RAMD_HD long long classify_block_decisions(const int *targets, int n_steps, int n, int n_groups, const int *group_size,
                                           unsigned char *masks, int *active, unsigned *generation) {
  const size_t stride = classify_mask_stride(n);
  long long trained = 0;
  for (int t = 0; t < n_steps; t++) {
    unsigned char *m = masks + (size_t)t * stride;
    active[t] = 0;
    for (size_t j = 0; j < stride; j++) {
      m[j] = 0;
    }
    for (int j = 0; j < n; j++) {
      const int *row = targets + ((size_t)t * n + j) * n_groups;
      for (int i = 0; i < n_groups; i++) {
        trained += classify_target_trains(row[i], group_size[i]);
      }
      m[j] = (unsigned char)classify_stream_active(row, n_groups, group_size);
      active[t] += m[j];
      if (generation && m[j]) {
        generation[j]++;
      }
    }
  }
  return trained;
}

/* Which blocks rnn_amd_set_classify_steps takes: 0, or the first thing that is wrong (the call prints the text and aborts,
 * as the set API does). */
enum {
  CLASSIFY_BLOCK_OK = 0,
  CLASSIFY_BLOCK_NULL = 1,     /* NULL features or targets */
  CLASSIFY_BLOCK_NO_STEPS = 2, /* n_steps < 1 */
  CLASSIFY_BLOCK_LD = 3,       /* ld < input_size: a row does not hold the features */
  CLASSIFY_BLOCK_NO_GROUPS = 4, /* n_groups < 1, or no offsets or sizes */
  CLASSIFY_BLOCK_GROUP = 5     /* a group that is empty or not within the outputs */
};
RAMD_HD int classify_block_refusal(int have_features, int have_targets, int n_steps, int ld, int input_size, int n_groups,
                                   const int *group_offset, const int *group_size, int output_size) {
  if (!have_features || !have_targets) {
    return CLASSIFY_BLOCK_NULL;
  }
  if (n_steps < 1) {
    return CLASSIFY_BLOCK_NO_STEPS;
  }
  if (ld < input_size) {
    return CLASSIFY_BLOCK_LD;
  }
  if (n_groups < 1 || !group_offset || !group_size) {
    return CLASSIFY_BLOCK_NO_GROUPS;
  }
  for (int i = 0; i < n_groups; i++) {
    if (group_offset[i] < 0 || group_size[i] < 1 || (long long)group_offset[i] + group_size[i] > output_size) {
      return CLASSIFY_BLOCK_GROUP;
    }
  }
  return CLASSIFY_BLOCK_OK;
}
RAMD_HD const char *classify_block_refusal_text(int refusal) {
  switch (refusal) {
  case CLASSIFY_BLOCK_OK: return "a block it takes";
  case CLASSIFY_BLOCK_NULL: return "no features or no targets";
  case CLASSIFY_BLOCK_NO_STEPS: return "fewer than one generation";
  case CLASSIFY_BLOCK_LD: return "rows too short for the features";
  case CLASSIFY_BLOCK_NO_GROUPS: return "no class groups";
  case CLASSIFY_BLOCK_GROUP: return "a class group outside the outputs";
  }
  return "?";
}

/* ---- balanced training (gstclassify.c:2190-2215, 2096-2104) ---- */

/* the probabilities of the generation that starts now, from the counts so far */
static inline void classify_balance_probabilities(const uint32_t *seen, int n_outputs, float bias, float *train_p) {
  uint32_t met = 0;
  for (int c = 0; c < n_outputs; c++) {
    met += seen[c];
  }
  const float share = 1.0f / (met + 1.0f);
  for (int c = 0; c < n_outputs; c++) {
    train_p[c] = powf(1.0f - seen[c] * share, bias);
  }
}

/* recur-rng.h:80-85: a float in [0, 1] from 64 random bits */
static inline float classify_unit_draw(uint64_t bits) { return (float)bits * (1.0f / ((float)0xfffffffffffffffeULL)); }

/* One generation's choice.  targets [channels][n_groups] are the labels; use[channel][group] becomes the label where the
 * pair trains and -1 where it does not, trains[channel] whether any of its groups does.  Without train_p every label
 * trains and nothing is drawn.  With it, every labelled pair -- channel-major, the groups of a channel in order -- counts
 * into seen, takes ONE draw (draw64(ctx): the next 64 bits of the prototype's generator) and trains iff
 * train_p[output] > the draw; then it counts into used.  Returns the number of pairs that train. */
typedef uint64_t (*classify_draw64)(void *ctx);
static inline int classify_balance_choose(int channels, int n_groups, const int *group_offset, const int *group_size,
                                          const int *targets, const float *train_p, uint32_t *seen, uint32_t *used,
                                          classify_draw64 draw64, void *ctx, int *use, unsigned char *trains) {
  int trained_groups = 0;
  for (int ch = 0; ch < channels; ch++) {
    trains[ch] = 0;
    for (int g = 0; g < n_groups; g++) {
      const int t = targets[(size_t)ch * n_groups + g];
      int take = classify_target_trains(t, group_size[g]);
      if (take && train_p) {
        const int out = group_offset[g] + t;
        seen[out]++;
        take = train_p[out] > classify_unit_draw(draw64(ctx));
        used[out] += (uint32_t)take;
      }
      use[(size_t)ch * n_groups + g] = take ? t : -1;
      trains[ch] |= (unsigned char)take;
      trained_groups += take;
    }
  }
  return trained_groups;
}

#endif
