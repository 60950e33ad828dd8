/* set_train.c -- the batched API's whole generations (include/recur_amd.h; gnu11 C): forward pass, loss, delta call and
 * update as ONE call (set_step: the text step, the multi-head step, the dense steps of rnnca and parrot), and the three
 * trainers that run many generations from one block on the device -- parrot's frames, rnnca's film, gstclassify's windows.
 * The pass and the delta call are set_api.c's, the losses set_loss.c's (set_internal.h); the exchange between ranks that a
 * step may end with is exchange.c's. */
#define RAMD_HIP_HOST 1
#include "set_internal.h"
#include "parrot_rule.h"
#include "automaton_train_rule.h"
#include "classify_train_rule.h"

static void char_step_deltas(RnnAmdSet *set, int i, RamdPendingDelta *defer) {
  RamdEngine *e = set->eng;
  ramd_set_check_text_pos(e, i, 0, "rnn_amd_set_char_step");
  if (ramd_text_top_ok(&e->sh)) {
    /* advance + hidden layer, then output layer, loss and top backprop in one launch -- or all of it in one
     * (fwd_top_plan.h: the north star's shape, RECUR_AMD_FWD_TOP=0 for the two) */
    const RamdHandover left = ramd_set_forward(set, RAMD_IN_TEXT, NULL, 0, i, NULL, 1, RAMD_FWD_FOR_TEXT_TOP);
    ramd_noise_ahead_offer(set, 0); /* no draws between this pass's noise and the next one's */
    if (!left.top_done) {
      ramd_launch_text_top(ramd_stream, &e->sh, &e->b, set->row0, set->n, left);
    }
    ramd_set_calc_deltas(set, 0, NULL, NULL, NULL, RAMD_TOP_DONE, NULL, 0, defer);
  } else {
    ramd_set_forward(set, RAMD_IN_TEXT, NULL, 0, i, NULL, 1, RAMD_FWD_WHOLE); /* advance + one-hot opinion */
    ramd_noise_ahead_offer(set, 0);
    ramd_launch_softmax_error(ramd_stream, &e->sh, &e->b, set->row0, set->n);
    ramd_set_calc_deltas(set, 0, NULL, NULL, NULL, 0, NULL, 0, defer);
  }
}

void rnn_amd_set_char_step_deltas(RnnAmdSet *set, int i) { char_step_deltas(set, i, NULL); }

/* With ONE rank the sum over the ranks is the rank's own sum and the sharded update is the whole update: the exchange
 * step -- the all-reduce, or the barriers and the peer-pointer update kernel -- is skipped and the generation is the
 * plain one (one-rank cost of either exchange path: 0; round 4: +4.8 us through RCCL, +11 us kernel-issued).
 * RECUR_AMD_DIST_ONE_RANK_EXCHANGE=1 keeps the exchange step in (tests and `bench.py --dist` exercise it on one GPU). */
static int one_rank_exchange_forced(void) {
  static int on = -1;
  if (on < 0) {
    const char *v = getenv("RECUR_AMD_DIST_ONE_RANK_EXCHANGE");
    on = v && *v == '1';
  }
  return on;
}

/* what a one-call generation does before its update: the text step (symbol i of the resident text), or a dense-input
 * generation with rnnca's loss (rnn_amd_set_dense_step_sigmoid_mse) */
typedef struct {
  int i;                /* text position, or -1: dense, or -2: the multi-head step */
  const float *inputs;  /* dense: [n][ld_inputs], the caller's host rows (with on_dev: device rows) */
  int ld_inputs;
  const float *targets; /* [n][ld], host rows or (on_dev) device rows: the first n_targets outputs */
  int ld, n_targets;
  RamdDenseLoss loss;   /* dense: rnnca's or parrot's */
  int advance;          /* dense: rnn_bptt_advance in front (parrot's train_net; rnn_amd_set_automaton_steps's `advance`) */
  int on_dev;           /* dense: inputs and targets are device rows (the many-step calls' blocks) */
  int stats;            /* dense, rnnca's: the squared error into the statistics (rnn_amd_set_automaton_steps alone) */
  /* the multi-head step (rnn_amd_set_multi_step_deltas's arguments) */
  const int *hot, *next, *target_class;
  int alphabet_len;
  float leakage;
} StepSpec;

static void step_deltas(RnnAmdSet *set, const StepSpec *sp, RamdPendingDelta *defer) {
  if (sp->i >= 0) {
    char_step_deltas(set, sp->i, defer);
  } else if (sp->i == -2) {
    ramd_set_multi_step_deltas(set, sp->hot, sp->next, sp->target_class, sp->alphabet_len, sp->leakage, 0, defer);
  } else {
    ramd_set_opinion_dense_loss(set, sp->loss, sp->inputs, sp->ld_inputs, sp->targets, sp->ld, sp->n_targets, sp->on_dev,
                                sp->advance, sp->stats);
    ramd_set_calc_deltas(set, 0, NULL, NULL, NULL, 0, NULL, 0, defer);
  }
}

static void set_step(RnnAmdSet *set, const StepSpec *sp, int learning_style, float momentum) {
  if (set->eng->xchg_world > 1 || (set->eng->xchg_world == 1 && one_rank_exchange_forced())) {
    /* deltas -> (barrier) -> sharded update with the sum over the ranks in it -> (barrier) */
    step_deltas(set, sp, NULL);
    rnn_amd_set_apply_exchange(set, learning_style, momentum);
    return;
  }
  /* the deltas go straight from the GEMM's K slabs into the update (and into ih_delta) when
   * nothing can look at them in between: library-owned storage, no log on the prototype */
  RamdPendingDelta pend = {0};
  const int dist = ramd_dist_active() && (rnn_amd_dist_world() > 1 || one_rank_exchange_forced());
  int fuse = !set->eng->delta_external && !set->nets[0]->log && !dist;
  if (dist) {
    ramd_halves_seen = 0;
    ramd_set_delta_half_hook(ramd_delta_half_ready, set->eng);
  }
  float mw, rate, ho_rate;
  const int method = ramd_update_rule(set->nets[0]->bptt, learning_style, momentum, &mw, &rate, &ho_rate);
  if (fuse && !set->eng->sh.bI && (method == RNN_MOMENTUM_WEIGHTED || method == RNN_ADAGRAD)) {
    /* the momentum rule (recur-nn.c:482-487, 653-676) or ADAGRAD (518-524, the multi-head trainer's rule): the
     * weight-delta GEMM may carry the update out in its own epilogue (kernels_bptt.hip: k_delta_direct), with the rates
     * and weights ramd_apply_learning would use (ADAGRAD's arithmetic reads neither the momentum nor its weight) */
    _Static_assert(RNN_MOMENTUM_WEIGHTED == 0 && RNN_ADAGRAD == 4, "RamdPendingDelta.fuse_method takes these two as they are");
    ramd_engine_need_dev(set->eng, RNN_AMD_WEIGHTS | RNN_AMD_MOMENTUMS);
    pend.fuse_want = 1;
    pend.fuse_method = method;
    pend.fuse_rate = rate;
    pend.fuse_ho_rate = ho_rate;
    pend.fuse_momentum = momentum;
    pend.fuse_mw = mw;
  }
  step_deltas(set, sp, fuse ? &pend : NULL);
  if (pend.fuse_done) { /* weights and momentum are updated, the delta arrays hold the sums */
    ramd_engine_dev_wrote(set->eng, RNN_AMD_WEIGHTS | RNN_AMD_MOMENTUMS | RNN_AMD_DELTAS);
    return;
  }
  if (dist) {
    /* the one exchange step of the path: this rank's deltas become the sum over all ranks'
     * streams (recur-nn.c:724-739 distributed), then the identical update everywhere */
    ramd_set_delta_half_hook(NULL, NULL);
    if (ramd_halves_seen == 3) { /* both halves are on their way: the update waits for them */
      HIP_OK(hipStreamWaitEvent(ramd_stream, ramd_half_summed[0], 0));
      HIP_OK(hipStreamWaitEvent(ramd_stream, ramd_half_summed[1], 0));
    } else { /* a shape the two-halves form does not take: one all-reduce behind the deltas */
      const int tev = ramd_timing_begin(ramd_stream, RAMD_T_XCHG);
      rnn_amd_dist_all_reduce(set->eng->b.ih_delta, set->eng->ih_size + set->eng->ho_size);
      ramd_timing_end(ramd_stream, tev);
    }
  }
  ramd_apply_learning(set->nets[0], learning_style, momentum, (pend.slab || pend.ho_slab) ? &pend : NULL, NULL);
}

/* the multi-head generation as ONE call: rnn_amd_set_multi_step_deltas (accumulate 0) + rnn_apply_learning -- knowing the
 * update that follows, the weight-delta GEMM carries it out in its own epilogue where the rule is ADAGRAD (the trainer's)
 * or the momentum rule: no optimiser launch (17 us of configs[3]'s 340) */
void rnn_amd_set_multi_step(RnnAmdSet *set, const int *hot, const int *next, const int *target_class, int alphabet_len,
                            float leakage, int learning_style, float momentum) {
  StepSpec sp = {.i = -2, .hot = hot, .next = next, .target_class = target_class, .alphabet_len = alphabet_len,
                 .leakage = leakage};
  set_step(set, &sp, learning_style, momentum);
}

void rnn_amd_set_char_step(RnnAmdSet *set, int i, int learning_style, float momentum) {
  StepSpec sp = {.i = i};
  set_step(set, &sp, learning_style, momentum);
}

/* rnnca's maybe_learn for every trainer (gstrnnca.c:693-740) as one call: see recur_amd.h */
void rnn_amd_set_dense_step_sigmoid_mse(RnnAmdSet *set, const float *inputs, int ld_inputs, const float *targets, int ld,
                                        int n, int learning_style, float momentum) {
  if (!inputs) {
    fprintf(stderr, "librecur_amd: rnn_amd_set_dense_step_sigmoid_mse needs the inputs\n");
    abort();
  }
  ramd_set_dense_loss_check(set, RAMD_DENSE_SIGMOID_MSE, "rnn_amd_set_sigmoid_mse_error", targets, ld, n); /* (as rnn_amd_set_opinion_sigmoid_mse) */
  rnn_bptt_clear_deltas(set->nets[0]); /* (lazy: the delta call below simply does not accumulate) */
  StepSpec sp = {.i = -1, .inputs = inputs, .ld_inputs = ld_inputs, .targets = targets, .ld = ld, .n_targets = n,
                 .loss = RAMD_DENSE_SIGMOID_MSE};
  set_step(set, &sp, learning_style, momentum);
}

/* parrot's maybe_learn for every channel at once (gstparrot.c:464-477, 487-554): see recur_amd.h */
static void dense_step_tanh(RnnAmdSet *set, const float *inputs, int ld_inputs, const float *targets, int ld, int n,
                            int on_dev, int learning_style, float momentum) {
  rnn_bptt_clear_deltas(set->nets[0]); /* (lazy: the delta call simply does not accumulate) */
  StepSpec sp = {.i = -1, .inputs = inputs, .ld_inputs = ld_inputs, .targets = targets, .ld = ld, .n_targets = n,
                 .loss = RAMD_DENSE_TANH_SLOPE, .advance = 1, .on_dev = on_dev};
  set_step(set, &sp, learning_style, momentum);
}

void rnn_amd_set_dense_step_tanh(RnnAmdSet *set, const float *inputs, int ld_inputs, const float *targets, int ld, int n,
                                 int learning_style, float momentum) {
  ramd_set_dense_loss_check(set, RAMD_DENSE_TANH_SLOPE, "rnn_amd_set_dense_step_tanh", targets, ld, n);
  if (!inputs || ld_inputs < set->eng->sh.input_size) {
    fprintf(stderr, "librecur_amd: rnn_amd_set_dense_step_tanh needs inputs (ld %d for %d)\n", ld_inputs,
            set->eng->sh.input_size);
    abort();
  }
  dense_step_tanh(set, inputs, ld_inputs, targets, ld, n, 0, learning_style, momentum);
}

/* n_steps of them from one block of frames, frame t + 1 being generation t's target and generation t + 1's input: the
 * block goes up once, the generations read their rows where they lie */
void rnn_amd_set_dense_steps_tanh(RnnAmdSet *set, const float *frames, int ld, int n_steps, int n, int learning_style,
                                  float momentum, int condition) {
  RamdEngine *e = set->eng;
  ramd_set_need_training(set, "rnn_amd_set_dense_steps_tanh");
  const int refusal = parrot_block_refusal(frames != NULL, n_steps, ld, e->sh.input_size, n, e->sh.output_size);
  if (refusal) { /* (the rule is parrot_rule.h's, where it is asked without a device) */
    fprintf(stderr, "librecur_amd: rnn_amd_set_dense_steps_tanh: %s (%d steps from frames %p of ld %d; %d inputs, %d of %d outputs)\n",
            parrot_block_refusal_text(refusal), n_steps, (const void *)frames, ld, e->sh.input_size, n, e->sh.output_size);
    abort();
  }
  const size_t frame = (size_t)set->n * ld;
  /* (a bottom layer keeps a host copy of the last stream's inputs per generation, rnn_amd_set_opinion: such a set takes
   * its rows from the host, generation by generation) */
  const int on_dev = !e->sh.bI;
  const float *base = frames;
  if (on_dev) {
    const size_t bytes = (size_t)(n_steps + 1) * frame * sizeof(float);
    float *d_frames = ramd_block_room(e, bytes);
    ramd_upload(d_frames, frames, bytes);
    base = d_frames;
  }
  for (int t = 0; t < n_steps; t++) {
    dense_step_tanh(set, base + (size_t)t * frame, ld, base + (size_t)(t + 1) * frame, ld, n, on_dev, learning_style,
                    momentum);
    if (condition) {
      rnn_condition_net(set->nets[0]); /* gstparrot.c:544-545: behind the update */
    }
  }
}

/* rnnca's trainer over a block of a film (gstrnnca.c:669-750; automaton_train_rule.h): the film, the positions and the
 * offset lists go up once, one launch gathers every generation's input and target rows from the film's bytes, and the
 * generations read their rows where they lie: see recur_amd.h */
void rnn_amd_set_automaton_steps(RnnAmdSet *set, const RnnAmdAutomaton *ca, const u8 *frames, const int *xy, int xy_per_step,
                                 int n_steps, int advance, int learning_style, float momentum, float momentum_soft_start,
                                 int condition) {
  AutomatonRule g = {0};
  if (ca) {
    g = (AutomatonRule){ca->width, ca->height, ca->offsets_y, ca->len_y, ca->offsets_c, ca->len_c, ca->len_pos, ca->edges};
  }
  RamdEngine *e = set ? set->eng : NULL;
  const int refusal = automaton_block_refusal(set != NULL, ca ? &g : NULL, frames != NULL, xy, xy_per_step, n_steps,
                                              set ? set->n : 0, e ? e->sh.input_size : 0, e ? e->sh.output_size : 0,
                                              e ? e->sh.bI : 0);
  if (refusal) { /* (the rule is automaton_train_rule.h's, where it is asked without a device) */
    fprintf(stderr, "librecur_amd: rnn_amd_set_automaton_steps: %s (%d steps of %d trainers on a grid of %d x %d)\n",
            automaton_block_refusal_text(refusal), n_steps, set ? set->n : 0, g.width, g.height);
    abort();
  }
  ramd_set_need_training(set, "rnn_amd_set_automaton_steps");
  const int n = set->n, in = e->sh.input_size;
  const size_t cells = (size_t)g.width * g.height;
  const size_t film = ((size_t)n_steps + 1) * 3 * cells, n_xy = 2 * (size_t)(xy_per_step ? n_steps : 1) * n;
  const size_t n_offy = 2 * (size_t)g.len_y, n_offc = 2 * (size_t)g.len_c;
  size_t bytes = 0;
  const size_t at_film = ramd_block_carve(&bytes, film);
  const size_t at_xy = ramd_block_carve(&bytes, n_xy * sizeof(int));
  const size_t at_off = ramd_block_carve(&bytes, (n_offy + n_offc) * sizeof(int));
  const size_t at_rows = ramd_block_carve(&bytes, (size_t)n_steps * n * in * sizeof(float));
  const size_t at_targets = ramd_block_carve(&bytes, (size_t)n_steps * n * 3 * sizeof(float));
  char *base = ramd_block_room(e, bytes);
  int *d_off = (int *)(base + at_off);
  ramd_upload_q(base + at_xy, xy, n_xy * sizeof(int));
  ramd_upload_q(d_off, g.offsets_y, n_offy * sizeof(int));
  ramd_upload_q(d_off + n_offy, g.offsets_c, n_offc * sizeof(int));
  ramd_upload(base + at_film, frames, film);
  g.offsets_y = d_off;
  g.offsets_c = d_off + n_offy;
  const RamdAutomatonTrainRows gather = {.g = g, .frames = (const u8 *)(base + at_film), .xy = (const int *)(base + at_xy),
                                         .xy_per_step = xy_per_step, .n_steps = n_steps, .n = n, .input_size = in,
                                         .rows = (float *)(base + at_rows), .targets = (float *)(base + at_targets)};
  ramd_launch_automaton_train_rows(ramd_stream, &gather);
  for (int t = 0; t < n_steps; t++) {
    rnn_bptt_clear_deltas(set->nets[0]); /* (lazy: the delta call simply does not accumulate) */
    const StepSpec sp = {.i = -1, .inputs = gather.rows + (size_t)t * n * in, .ld_inputs = in,
                         .targets = gather.targets + (size_t)t * n * 3, .ld = 3, .n_targets = 3, .loss = RAMD_DENSE_SIGMOID_MSE,
                         .advance = advance != 0, .on_dev = 1, .stats = 1};
    set_step(set, &sp, learning_style, automaton_train_momentum(set->nets[0]->generation, momentum, momentum_soft_start));
    if (condition) {
      rnn_condition_net(set->nets[0]); /* gstrnnca.c:739: behind the update */
    }
  }
}

/* gstclassify's trainer over a block of windows (maybe_learn, gstclassify.c:2180-2257; classify_train_rule.h): see
 * recur_amd.h.  One generation from the caller's host rows, the gate decided by reading the summed error back: what the
 * block call does where the block cannot stay on the device (a bottom layer's host copy of its inputs, noise drawn in
 * front of every pass, an exchange or a group of ranks behind every update).  trains: room for a flag per stream */
static void classify_generation_host(RnnAmdSet *set, const float *features, int ld, const int *targets, int n_groups,
                                     const int *group_offset, const int *group_size, const float *error_weight,
                                     int learning_style, float momentum_soft_start, int condition, u8 *trains) {
  RecurNN *net = set->nets[0];
  rnn_bptt_clear_deltas(net);
  RnnAmdStats before, after;
  const int together = net->presynaptic_noise == 0.0f; /* (a noisy pass draws first, as in train_channel) */
  if (!together) {
    rnn_amd_set_opinion(set, features, ld, NULL);
  }
  rnn_amd_set_read_stats(set, &before, 0);
  if (together) {
    rnn_amd_set_opinion_grouped_softmax(set, features, ld, n_groups, group_offset, group_size, targets, error_weight, trains);
  } else {
    rnn_amd_set_grouped_softmax_error(set, n_groups, group_offset, group_size, targets, error_weight, trains);
  }
  const int any = memchr(trains, 1, (size_t)set->n) != NULL;
  if (any) {
    rnn_amd_set_calc_deltas(set, 1, NULL, trains); /* adds to the cleared deltas */
  }
  rnn_amd_set_advance(set);
  if (any) {
    rnn_amd_set_read_stats(set, &after, 0);
    if (after.error - before.error != 0.0) { /* the reference's `if (err_sum)` */
      rnn_apply_learning(net, learning_style,
                         rnn_calculate_momentum_soft_start(net->generation, net->bptt->momentum, momentum_soft_start));
    }
  }
  if (condition) {
    rnn_condition_net(net);
  }
}

void rnn_amd_set_classify_steps(RnnAmdSet *set, const float *features, int ld, const int *targets, int n_steps, int n_groups,
                                const int *group_offset, const int *group_size, const float *error_weight,
                                int learning_style, float momentum_soft_start, int condition) {
  if (!set) {
    fprintf(stderr, "librecur_amd: rnn_amd_set_classify_steps without a set\n");
    abort();
  }
  RamdEngine *e = set->eng;
  ramd_set_need_training(set, "rnn_amd_set_classify_steps");
  const int width = e->sh.bI ? e->sh.b_in : e->sh.input_size; /* (a bottom layer takes the features) */
  const int refusal = classify_block_refusal(features != NULL, targets != NULL, n_steps, ld, width, n_groups, group_offset,
                                             group_size, e->sh.output_size);
  if (refusal) { /* (the rule is classify_train_rule.h's, where it is asked without a device) */
    fprintf(stderr, "librecur_amd: rnn_amd_set_classify_steps: %s (%d steps, rows of %d for %d inputs, %d groups in %d outputs)\n",
            classify_block_refusal_text(refusal), n_steps, ld, width, n_groups, e->sh.output_size);
    abort();
  }
  RecurNN *net = set->nets[0];
  const int n = set->n;
  const size_t stride = classify_mask_stride(n);
  if (e->sh.bI || net->presynaptic_noise != 0.0f || e->xchg_world || rnn_amd_dist_world() > 1) {
    u8 *trains = ramd_zalloc(stride);
    for (int t = 0; t < n_steps; t++) {
      classify_generation_host(set, features + (size_t)t * n * ld, ld, targets + (size_t)t * n * n_groups, n_groups,
                               group_offset, group_size, error_weight, learning_style, momentum_soft_start, condition, trains);
    }
    free(trains);
    return;
  }
  /* the block: features, then -- staged on the host as one piece -- targets, masks, gate words (zero), groups, weights */
  const size_t n_feat = (size_t)n_steps * n * ld, n_tg = (size_t)n_steps * n * n_groups;
  const size_t n_weights = error_weight ? (size_t)e->sh.output_size : 0;
  size_t bytes = 0;
  const size_t at_feat = ramd_block_carve(&bytes, n_feat * sizeof(float));
  const size_t at_tg = ramd_block_carve(&bytes, n_tg * sizeof(int));
  const size_t at_masks = ramd_block_carve(&bytes, (size_t)n_steps * stride);
  const size_t at_gates = ramd_block_carve(&bytes, (size_t)n_steps * sizeof(unsigned));
  const size_t at_groups = ramd_block_carve(&bytes, (size_t)2 * n_groups * sizeof(int));
  const size_t at_weights = ramd_block_carve(&bytes, n_weights * sizeof(float));
  char *base = ramd_block_room(e, bytes);
  char *tail = ramd_zalloc(bytes - at_tg); /* (zeroed: the gate words, the masks' padding) */
  u8 *masks = (u8 *)(tail + (at_masks - at_tg));
  int *active = ramd_zalloc((size_t)n_steps * sizeof(int));
  memcpy(tail, targets, n_tg * sizeof(int));
  classify_block_decisions(targets, n_steps, n, n_groups, group_size, masks, active, NULL);
  memcpy(tail + (at_groups - at_tg), group_offset, (size_t)n_groups * sizeof(int));
  memcpy(tail + (at_groups - at_tg) + (size_t)n_groups * sizeof(int), group_size, (size_t)n_groups * sizeof(int));
  if (error_weight) {
    memcpy(tail + (at_weights - at_tg), error_weight, n_weights * sizeof(float));
  }
  ramd_upload_q(base + at_feat, features, n_feat * sizeof(float));
  ramd_upload(base + at_tg, tail, bytes - at_tg);
  const float *d_feat = (const float *)(base + at_feat);
  const int *d_tg = (const int *)(base + at_tg);
  unsigned *d_gates = (unsigned *)(base + at_gates);
  RamdTopLoss groups = {.kind = RAMD_TOP_CLASS_GROUPS, .ngroups = n_groups, .goff = (const int *)(base + at_groups),
                        .weight = error_weight ? (const float *)(base + at_weights) : NULL};
  groups.gsize = groups.goff + n_groups;
  int largest = 1;
  for (int i = 0; i < n_groups; i++) {
    largest = RAMD_MAX(largest, group_size[i]);
  }
  for (int t = 0; t < n_steps; t++) {
    rnn_bptt_clear_deltas(net); /* (lazy: the delta call simply does not accumulate) */
    const float *x = d_feat + (size_t)t * n * ld;
    groups.gt = d_tg + (size_t)t * n * n_groups;
    groups.gate = d_gates + t;
    const u8 *mask = masks + (size_t)t * stride;
    /* generation t - 1's rnn_bptt_advance rides in this forward launch; the last one's follows the loop */
    const int advance = t > 0;
    /* the one-launch top where rnn_amd_set_opinion_grouped_softmax takes it: its output layer sums in another order than
     * the separate kernels', and the block keeps the bits of the loop of rnn_amd_classify_generation at every set size */
    if (ramd_set_dense_top_ok(set, x, RAMD_TOP_CLASS_GROUPS) && n % 4 == 0) {
      ramd_set_class_group_top(set, "rnn_amd_set_classify_steps", x, ld, advance, &groups, mask);
    } else {
      ramd_set_forward(set, RAMD_IN_DENSE, x, ld, 0, NULL, advance, RAMD_FWD_WHOLE);
      ramd_launch_grouped_softmax_error(ramd_stream, &e->sh, &e->b, set->row0, n, n_groups, largest, groups.goff, groups.gsize,
                                        groups.gt, groups.weight, groups.gate);
      ramd_set_streams_dev_wrote(set);
    }
    if (active[t]) {
      /* never with the delta GEMM's update epilogue: the gate needs the optimiser launch of its own */
      ramd_set_calc_deltas(set, 1, NULL, mask, (const u8 *)(base + at_masks) + (size_t)t * stride, 0, NULL, 0, NULL);
      ramd_apply_learning(net, learning_style,
                          rnn_calculate_momentum_soft_start(net->generation, net->bptt->momentum, momentum_soft_start), NULL,
                          d_gates + t);
    }
    if (condition) {
      rnn_condition_net(net);
    }
  }
  rnn_amd_set_advance(set);
  free(active);
  free(tail);
}

