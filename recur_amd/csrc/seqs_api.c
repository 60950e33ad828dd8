/* seqs_api.c -- many dense feature sequences against one net in one batched device run (gnu11 C):
 * rnn_amd_run_sequences, the batched form of emit_opinions' loop body (gstclassify.c:2259-2292: rnn_opinion on the
 * window's features, softmax_best_guess per class group) and, without groups, of a plain loop of rnn_opinion on dense rows
 * (rnnca, parrot).  It is texts_api.c with frames where that has symbols: every sequence gets a forward-only state row of
 * the engine's own, texts_plan.h orders the rows and cuts the waves, between two forward passes of the rows there is one
 * launch (k_seqs_step, kernels_rows.hip) that turns the outputs just computed into answers and winners and builds the
 * input rows of the next pass, and the states travel as texts_states.h says.  What differs is the staging: a frame is
 * 4 * input_size bytes, so a wave runs in segments (seqs_plan.h) -- per segment the frames of the rows that still run go up
 * in one copy, the launches run, the answers and the winners come back in one copy each, and there is one
 * synchronisation.  The state rows carry over between the segments by themselves.  The net the caller passes is read --
 * its weights, its hidden row -- and not written. */
#define RAMD_HIP_HOST 1
#include <limits.h>
#include "rnn_host.h"
#include "seqs_plan.h"
#include "texts_states.h"

#define WHO "rnn_amd_run_sequences"

/* the refusals, which need no device: -1 with a line on stderr, else 0.  covered[output_size] (the caller's, zeroed)
 * is left with 1 on every column that lies in a group */
static int seqs_refused(const RecurNN *net, const float *const *inputs, const int *n_frames, int n_seqs, int ld_inputs,
                        int n_groups, const int *group_offset, const int *group_size, float *const *answers,
                        u8 *const *winners, u8 *covered) {
  if (ld_inputs < net->input_size) {
    fprintf(stderr, "librecur_amd: " WHO ": rows of %d floats do not hold %d inputs\n", ld_inputs, net->input_size);
    return -1;
  }
  if (n_groups > 0 && (!group_offset || !group_size)) {
    fprintf(stderr, "librecur_amd: " WHO ": a NULL array for %d class groups\n", n_groups);
    return -1;
  }
  for (int g = 0; g < n_groups; g++) {
    const int o = group_offset[g], n = group_size[g];
    if (o < 0 || n < 1 || o > net->output_size || n > net->output_size - o) {
      fprintf(stderr, "librecur_amd: " WHO ": class group %d (%d classes from output %d) leaves the %d outputs\n", g, n, o,
              net->output_size);
      return -1;
    }
    for (int i = o; i < o + n; i++) {
      if (covered[i]) {
        fprintf(stderr, "librecur_amd: " WHO ": class group %d overlaps another at output %d\n", g, i);
        return -1;
      }
      covered[i] = 1;
    }
    if (winners && n > 256) {
      fprintf(stderr, "librecur_amd: " WHO ": a winner among %d classes does not fit a byte\n", n);
      return -1;
    }
  }
  if (winners && n_groups == 0) {
    fprintf(stderr, "librecur_amd: " WHO ": winners are wanted and there is no class group\n");
    return -1;
  }
  if (n_seqs > 0 && (!inputs || !n_frames || !answers)) {
    fprintf(stderr, "librecur_amd: " WHO ": a NULL array for %d sequences\n", n_seqs);
    return -1;
  }
  for (int k = 0; k < n_seqs; k++) {
    if (n_frames[k] < 0 || n_frames[k] == INT_MAX) {
      fprintf(stderr, "librecur_amd: " WHO ": sequence %d has %d frames\n", k, n_frames[k]);
      return -1;
    }
    if (n_frames[k] >= 1 && (!inputs[k] || !answers[k] || (winners && !winners[k]))) {
      fprintf(stderr, "librecur_amd: " WHO ": sequence %d has a NULL array\n", k);
      return -1;
    }
  }
  return 0;
}

/* what a call wants and what its class groups are, on both sides */
typedef struct SeqsCall {
  const float *const *inputs;
  int ld_inputs;
  float *const *answers;
  u8 *const *winners;
  const float *h_in;
  float *h_out;
  int F; /* frames per segment */
  int n_groups, largest, n_gap;
  int *d_goff, *d_gsize, *d_gap;
} SeqsCall;

/* the staging buffers, with room for the plan's largest segment (the first of the first wave); the h_* ones are the host
 * sides and stay untouched from a segment's copies to its synchronisation */
typedef struct SeqsBuffers {
  float *h_in, *d_in;   /* the segment's frames   */
  float *h_ans, *d_ans; /* its answers            */
  u8 *h_win, *d_win;    /* its winners, or NULL   */
  unsigned long long *h_off, *d_off;
  int *count;
  float *h_state; /* [rows][H] the wave's states on their way in and out, or NULL */
} SeqsBuffers;

static void run_wave(const RamdRows *rows, const TextsPlan *plan, int w, const SeqsCall *c, const SeqsBuffers *sb) {
  RamdEngine *e = rows->e;
  const RamdShape *s = &e->sh;
  const TextsWave *wave = &plan->waves[w];
  const int n = wave->nrows;
  const size_t in_w = (size_t)s->input_size, out_w = (size_t)s->output_size;
  RamdSeqsStep step = {.in = sb->d_in, .ans = sb->d_ans, .win = sb->d_win, .off = sb->d_off, .goff = c->d_goff,
                       .gsize = c->d_gsize, .gap = c->d_gap, .row0 = rows->r0, .n_groups = c->n_groups, .n_gap = c->n_gap,
                       .largest = c->largest};
  step.hid0 = ramd_rows_states_in(rows, plan, w, c->h_in, sb->h_state); /* (the wave's first launch: t0 + i == 0) */
  const int n_segments = seqs_plan_segments(plan, w, c->F);
  for (int q = 0; q < n_segments; q++) {
    int t0, frames, live;
    const size_t total = (size_t)seqs_plan_segment(plan, w, q, c->F, &t0, &frames, &live, sb->count, sb->h_off);
    for (int j = 0; j < live; j++) {
      const float *src = c->inputs[plan->order[wave->row0 + j]] + (size_t)t0 * c->ld_inputs;
      float *dst = sb->h_in + (size_t)sb->h_off[j] * in_w;
      if ((size_t)c->ld_inputs == in_w) {
        memcpy(dst, src, (size_t)sb->count[j] * in_w * sizeof(float));
      } else {
        for (int i = 0; i < sb->count[j]; i++) {
          memcpy(dst + (size_t)i * in_w, src + (size_t)i * c->ld_inputs, in_w * sizeof(float));
        }
      }
    }
    ramd_h2d(sb->d_in, sb->h_in, total * in_w * sizeof(float));
    ramd_h2d(sb->d_off, sb->h_off, (size_t)n * sizeof(unsigned long long));
    step.a_feed = 0;
    for (int i = 0; i <= frames; i++) {
      step.t_score = i - 1;
      step.a_score = step.a_feed; /* the rows whose frame i - 1 waits to be scored */
      step.t_feed = i;
      step.a_feed = i < frames ? texts_plan_active(plan, w, t0 + i) : 0;
      ramd_launch_seqs_step(ramd_stream, s, &e->b, &step);
      step.hid0 = NULL;
      if (step.a_feed) {
        ramd_rows_forward(rows, step.a_feed);
      }
    }
    ramd_d2h(sb->h_ans, sb->d_ans, total * out_w * sizeof(float));
    if (c->winners) {
      ramd_d2h(sb->h_win, sb->d_win, total * (size_t)c->n_groups);
    }
    if (q == n_segments - 1) { /* a row's last forward pass was its last writer */
      ramd_rows_states_out(rows, n, c->h_out ? sb->h_state : NULL);
    }
    ramd_dsync(); /* the segment's one synchronisation */
    for (int j = 0; j < live; j++) {
      const int k = plan->order[wave->row0 + j];
      memcpy(c->answers[k] + (size_t)t0 * out_w, sb->h_ans + (size_t)sb->h_off[j] * out_w,
             (size_t)sb->count[j] * out_w * sizeof(float));
      if (c->winners) {
        memcpy(c->winners[k] + (size_t)t0 * c->n_groups, sb->h_win + (size_t)sb->h_off[j] * c->n_groups,
               (size_t)sb->count[j] * c->n_groups);
      }
    }
  }
  if (c->h_out) {
    texts_states_unpack(plan, w, sb->h_state, s->H, c->h_out);
  }
}

int rnn_amd_run_sequences(RecurNN *net, const float *const *inputs, const int *n_frames, int n_seqs, int ld_inputs,
                          int n_groups, const int *group_offset, const int *group_size, const float *h_in, float *h_out,
                          int segment_frames, float *const *answers, u8 *const *winners) {
  if (!net || n_seqs < 0 || n_groups < 0) {
    fprintf(stderr, "librecur_amd: " WHO ": %d sequences, %d class groups\n", n_seqs, n_groups);
    return -1;
  }
  if (ramd_texts_net_refused(WHO, net, 0)) {
    return -1;
  }
  u8 *covered = calloc((size_t)net->output_size + 1, 1);
  if (!covered) {
    fprintf(stderr, "librecur_amd: " WHO ": out of memory\n");
    return -1;
  }
  if (seqs_refused(net, inputs, n_frames, n_seqs, ld_inputs, n_groups, group_offset, group_size, answers, winners, covered)) {
    free(covered);
    return -1;
  }
  TextsPlan plan = {0};
  int *lens = malloc((size_t)(n_seqs > 0 ? n_seqs : 1) * sizeof(int)); /* (the states' rule counts symbols) */
  int *groups = malloc((size_t)(2 * n_groups + net->output_size + 1) * sizeof(int));
  if (!lens || !groups || seqs_plan_make(&plan, n_frames, n_seqs, TEXTS_PLAN_WIDTH, lens)) {
    fprintf(stderr, "librecur_amd: " WHO ": out of memory planning %d sequences\n", n_seqs);
    goto fail;
  }
  if (ramd_texts_fill_rowless(net, lens, n_seqs, plan.n_rows, h_in, h_out)) {
    fprintf(stderr, "librecur_amd: " WHO ": out of memory\n");
    goto fail;
  }
  if (plan.n_rows == 0) { /* no sequence has a frame: no device is asked for */
    free(lens);
    free(groups);
    free(covered);
    return 0;
  }
  SeqsCall c = {.inputs = inputs, .ld_inputs = ld_inputs, .answers = answers, .winners = winners, .h_in = h_in,
                .h_out = h_out, .n_groups = n_groups};
  c.F = seqs_plan_segment_frames(segment_frames, net->input_size, TEXTS_PLAN_WIDTH);
  int *gap = groups + 2 * n_groups;
  for (int g = 0; g < n_groups; g++) {
    groups[g] = group_offset[g];
    groups[n_groups + g] = group_size[g];
    c.largest = RAMD_MAX(c.largest, group_size[g]);
  }
  for (int i = 0; i < net->output_size; i++) {
    if (!covered[i]) {
      gap[c.n_gap++] = i;
    }
  }
  const int widest = plan.waves[0].nrows;
  RamdRows rows;
  ramd_rows_open(&rows, net, widest);
  const size_t room = (size_t)seqs_plan_largest(&plan, c.F); /* frames of the largest segment */
  const size_t n_ints = (size_t)(2 * n_groups + c.n_gap);
  c.d_goff = ramd_rows_dev(&rows, (n_ints ? n_ints : 1) * sizeof(int));
  c.d_gsize = c.d_goff + n_groups;
  c.d_gap = c.d_goff + 2 * n_groups;
  if (n_ints) {
    ramd_h2d(c.d_goff, groups, n_ints * sizeof(int));
  }
  SeqsBuffers sb = {0};
  sb.h_in = ramd_rows_host(&rows, room * (size_t)net->input_size * sizeof(float));
  sb.d_in = ramd_rows_dev(&rows, room * (size_t)net->input_size * sizeof(float));
  sb.h_ans = ramd_rows_host(&rows, room * (size_t)net->output_size * sizeof(float));
  sb.d_ans = ramd_rows_dev(&rows, room * (size_t)net->output_size * sizeof(float));
  if (winners) {
    sb.h_win = ramd_rows_host(&rows, room * (size_t)n_groups);
    sb.d_win = ramd_rows_dev(&rows, room * (size_t)n_groups);
  }
  sb.h_off = ramd_rows_host(&rows, (size_t)widest * sizeof(unsigned long long));
  sb.d_off = ramd_rows_dev(&rows, (size_t)widest * sizeof(unsigned long long));
  sb.count = ramd_rows_host(&rows, (size_t)widest * sizeof(int));
  if (h_in || h_out) {
    sb.h_state = ramd_rows_host(&rows, (size_t)widest * rows.e->sh.H * sizeof(float));
  }
  for (int w = 0; w < plan.n_waves; w++) {
    run_wave(&rows, &plan, w, &c, &sb);
  }
  ramd_rows_close(&rows);
  free(lens);
  free(groups);
  free(covered);
  texts_plan_free(&plan);
  return 0;
fail:
  free(lens);
  free(groups);
  free(covered);
  texts_plan_free(&plan);
  return -1;
}
