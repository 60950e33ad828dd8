/* set_loss.c -- the batched API's losses: what lies between a set's forward pass and its delta call (include/recur_amd.h;
 * gnu11 C).  The softmax loss, gstclassify's class groups, the multi-head loss with its ranges, and the dense losses
 * (rnnca's sigmoid + squared error, parrot's tanh + slope error), each behind a finished pass and -- where one top launch
 * can carry output layer, loss and top backprop -- as opinion plus loss.  The pass and the delta call are set_api.c's, whole
 * generations set_train.c's (set_internal.h). */
#define RAMD_HIP_HOST 1
#include "set_internal.h"

void rnn_amd_set_softmax_error(RnnAmdSet *set, const int *target) {
  RamdEngine *e = set->eng;
  ramd_top_done_clear(e);
  ramd_set_need_training(set, "rnn_amd_set_softmax_error");
  ramd_set_streams_to_dev(set);
  if (target) {
    ramd_upload(e->b.target + set->row0, target, set->n * sizeof(int));
  }
  ramd_launch_softmax_error(ramd_stream, &e->sh, &e->b, set->row0, set->n);
  ramd_set_streams_dev_wrote(set);
}

/* the staging buffer of the losses' targets and class groups (d_group) has room for `bytes`.  Per generation, and live
 * during a block trainer's call: not the block buffer (ramd_block_room) */
static void group_room(RamdEngine *e, size_t bytes) {
  if (bytes > e->d_group_bytes) {
    ramd_dsync();
    ramd_dev_free(e->d_group);
    e->d_group = ramd_dev_alloc(bytes);
    e->d_group_bytes = bytes;
  }
}

/* ---- gstclassify's class groups ---- */

/* The class groups of gstclassify's loss on the device, for its launch: every group lies within the outputs (or the call
 * aborts), then one staging block -- offsets, sizes, targets, then the weights (or NULL) -- whose uploads are queued and
 * leave with the caller's next flush; `inputs` (or NULL): the call's dense input rows, which travel in front of them.
 * trained (or NULL): a stream is trained if any of its groups has a usable target.  -> the groups as the top launch takes
 * them (kind, the device arrays), *largest the largest group's size */
static RamdTopLoss class_groups_stage(RnnAmdSet *set, const float *inputs, int ld_inputs, int n_groups,
                                      const int *group_offset, const int *group_size, const int *targets,
                                      const float *error_weight, u8 *trained, int *largest) {
  RamdEngine *e = set->eng;
  const RamdShape *s = &e->sh;
  *largest = 1;
  for (int i = 0; i < n_groups; i++) {
    if (group_offset[i] < 0 || group_size[i] < 1 || group_offset[i] + group_size[i] > s->output_size) {
      fprintf(stderr, "librecur_amd: class group %d (%d + %d) outside the %d outputs\n", i, group_offset[i],
              group_size[i], s->output_size);
      abort();
    }
    *largest = RAMD_MAX(*largest, group_size[i]);
  }
  const size_t ints = (size_t)2 * n_groups + (size_t)set->n * n_groups;
  group_room(e, ints * sizeof(int) + (error_weight ? (size_t)s->output_size * sizeof(float) : 0));
  int *d = (int *)e->d_group;
  RamdTopLoss g = {.kind = RAMD_TOP_CLASS_GROUPS, .ngroups = n_groups, .goff = d, .gsize = d + n_groups, .gt = d + 2 * n_groups};
  if (inputs) {
    ramd_upload_rows_q(e->d_dense, inputs, ld_inputs * sizeof(float), s->input_size * sizeof(float), set->n, 0);
  }
  ramd_upload_q(d, group_offset, n_groups * sizeof(int));
  ramd_upload_q(d + n_groups, group_size, n_groups * sizeof(int));
  ramd_upload_q(d + 2 * n_groups, targets, (size_t)set->n * n_groups * sizeof(int));
  if (error_weight) {
    g.weight = (float *)(d + ints);
    ramd_upload_q((float *)(d + ints), error_weight, (size_t)s->output_size * sizeof(float));
  }
  for (int j = 0; trained && j < set->n; j++) {
    trained[j] = 0;
    for (int i = 0; i < n_groups; i++) {
      int t = targets[(size_t)j * n_groups + i];
      trained[j] |= (t >= 0 && t < group_size[i]);
    }
  }
  return g;
}

/* gstclassify's loss for the whole set (gstclassify.c:2070-2119), see recur_amd.h */
void rnn_amd_set_grouped_softmax_error(RnnAmdSet *set, int n_groups, const int *group_offset,
                                       const int *group_size, const int *targets,
                                       const float *error_weight, u8 *trained) {
  RamdEngine *e = set->eng;
  ramd_set_need_training(set, "rnn_amd_set_grouped_softmax_error");
  ramd_top_done_clear(e);
  ramd_set_streams_to_dev(set);
  int largest;
  const RamdTopLoss g = class_groups_stage(set, NULL, 0, n_groups, group_offset, group_size, targets, error_weight, trained,
                                           &largest);
  /* the caller hands the flags to rnn_amd_set_calc_deltas next (gstclassify.c:2120-2127): they travel with this call's
   * uploads, and that call finds them in place (ramd_set_active_mask_to_dev) */
  if (trained && set->n % 4 == 0 && !set->fwd_only) {
    ramd_set_active_mask_to_dev(e, trained, set->n, 1);
  }
  ramd_mail_in_flush();
  ramd_launch_grouped_softmax_error(ramd_stream, &e->sh, &e->b, set->row0, set->n, n_groups, largest, g.goff, g.gsize, g.gt,
                                    g.weight, NULL);
  ramd_set_streams_dev_wrote(set);
}

/* dense inputs -> hidden layer's sums only (they stay in the workspace for ramd_launch_dense_top of this kind); 0 where
 * that launch cannot follow */
int ramd_set_dense_top_ok(RnnAmdSet *set, const float *inputs, int kind) {
  RamdEngine *e = set->eng;
  return inputs && !set->fwd_only && !e->sh.bI && ramd_dense_top_ok(&e->sh, kind) &&
         set->nets[0]->presynaptic_noise == 0.0f && set->nets[0]->bptt;
}

/* The class-group top: the pass of the device rows d_inputs for the dense top (advance: rnn_bptt_advance first), the one
 * launch of output layer, class-group loss and top backprop (groups: staged on the device, with the generation's gate word
 * or none), and the book-keeping that lets the delta call skip the backprop for exactly the streams `trained` flags.  For a
 * set ramd_set_dense_top_ok takes; `what` names the caller should the launch decline after all */
void ramd_set_class_group_top(RnnAmdSet *set, const char *what, const float *d_inputs, int ld_inputs, int advance,
                              const RamdTopLoss *groups, const u8 *trained) {
  RamdEngine *e = set->eng;
  const RamdHandover left = ramd_set_forward(set, RAMD_IN_DENSE, d_inputs, ld_inputs, 0, NULL, advance, RAMD_FWD_FOR_DENSE_TOP);
  if (!ramd_launch_dense_top(ramd_stream, &e->sh, &e->b, set->row0, set->n, left, groups)) {
    fprintf(stderr, "librecur_amd: %s: the top launch declined a shape it had accepted\n", what);
    abort();
  }
  ramd_set_streams_dev_wrote(set);
  ramd_top_done_set(e, set->row0, set->n, 1);
  if (!e->top_done_mask) {
    e->top_done_mask = ramd_zalloc((size_t)e->sh.Scap + 4);
  }
  memcpy(e->top_done_mask, trained, (size_t)set->n); /* (a copy of its own: active_host follows whatever mask is sent next) */
}

void rnn_amd_set_opinion_grouped_softmax(RnnAmdSet *set, const float *inputs, int ld_inputs, int n_groups,
                                         const int *group_offset, const int *group_size, const int *targets,
                                         const float *error_weight, u8 *trained) {
  RamdEngine *e = set->eng;
  if (!ramd_set_dense_top_ok(set, inputs, RAMD_TOP_CLASS_GROUPS) || !trained || set->n % 4 != 0) {
    rnn_amd_set_opinion(set, inputs, ld_inputs, NULL);
    rnn_amd_set_grouped_softmax_error(set, n_groups, group_offset, group_size, targets, error_weight, trained);
    return;
  }
  ramd_set_need_training(set, "rnn_amd_set_opinion_grouped_softmax");
  int largest;
  const RamdTopLoss g = class_groups_stage(set, inputs, ld_inputs, n_groups, group_offset, group_size, targets, error_weight,
                                           trained, &largest);
  ramd_set_active_mask_to_dev(e, trained, set->n, 1); /* (for the delta call that follows: travels with the rest) */
  ramd_set_class_group_top(set, "rnn_amd_set_opinion_grouped_softmax", e->d_dense, e->sh.input_size, 0, &g, trained);
}

/* ---- the multi-head loss ---- */

/* The multi-head text model for the whole set, per generation: what
 * charmodel-multi-predict.c:244-256 does per net (rnn_bptt_advance, multi_softmax_error
 * with its one_hot_opinion, rnn_bptt_calc_deltas with the error ranges), stream j
 * accumulating on top of stream j - 1.  The loss half leaves o_error and one range list
 * per stream on the device; the deltas half consumes them.  In between the caller may
 * apply the previous batch's deltas, as text_train does (244-252). */
static const int MULTI_RANGE_STRIDE = RAMD_MULTI_RANGE_STRIDE; /* 2 x (64 + 1) ints and the head bits */

static int multi_heads(RamdEngine *e, int alphabet_len) {
  const RamdShape *s = &e->sh;
  int n_classes = alphabet_len > 0 ? s->output_size / alphabet_len : 0;
  if (alphabet_len < 1 || n_classes < 1 || n_classes > 64) {
    fprintf(stderr, "librecur_amd: %d outputs as heads of %d: 1 to 64 heads are supported\n",
            s->output_size, alphabet_len);
    abort();
  }
  if (!e->d_mranges) {
    e->d_mranges = ramd_dev_alloc((size_t)s->Scap * MULTI_RANGE_STRIDE * sizeof(int));
    e->d_mclass = ramd_dev_alloc((size_t)s->Scap * sizeof(int));
  }
  /* the sparse top backprop's partial products, one row of h_size per (stream, head): 53 MB at 256 streams of 50
   * heads and 1024 hidden units; sets too large for that keep the one-GEMM form (k_top_backprop_heads) */
  size_t part = (size_t)s->Scap * n_classes * s->H;
  if (alphabet_len >= 24 && alphabet_len <= 128 && part > e->b.mheads_part_floats && part * sizeof(float) <= ((size_t)2 << 30)) {
    ramd_dev_free(e->b.mheads_part);
    e->b.mheads_part = ramd_dev_alloc(part * sizeof(float));
    e->b.mheads_part_floats = part;
  }
  return n_classes;
}

/* the loss after the opinion: b.target holds each stream's next symbol.  offered: the early offer to generate the next
 * pass's noise has been made (ramd_set_multi_step_deltas) */
static void multi_loss(RnnAmdSet *set, const int *target_class, int alphabet_len, int n_classes,
                       float leakage, int offered) {
  RamdEngine *e = set->eng;
  e->mheads_alen = alphabet_len;
  e->b.mheads_alen = alphabet_len;
  if (target_class) {
    ramd_upload(e->d_mclass + set->row0, target_class, set->n * sizeof(int));
    noise_ahead_classes(&e->ahead, target_class, set->n, n_classes);
  }
  noise_ahead_loss(&e->ahead, n_classes); /* the leak decisions are draws from the streams' generators */
  /* u64 threshold = leakage * UINT64_MAX (charmodel-multi-predict.c:27): float arithmetic */
  float tf = leakage * (float)UINT64_MAX;
  unsigned long long threshold = tf >= 18446744073709551615.0f ? UINT64_MAX : (unsigned long long)tf;
  ramd_launch_multi_softmax_error(ramd_stream, &e->sh, &e->b, set->row0, set->n, alphabet_len, n_classes,
                                  threshold, e->d_mclass + set->row0,
                                  e->d_mranges + (size_t)set->row0 * MULTI_RANGE_STRIDE,
                                  MULTI_RANGE_STRIDE);
  ramd_set_streams_dev_wrote(set);
  if (!offered) {
    ramd_noise_ahead_offer(set, 0); /* the next draws are the next forward pass's noise */
  }
}

static void multi_calc_deltas(RnnAmdSet *set, int accumulate, RamdPendingDelta *defer) {
  RamdEngine *e = set->eng;
  ramd_set_need_training(set, "rnn_amd_set_multi_calc_deltas");
  if (!e->d_mranges) {
    fprintf(stderr, "librecur_amd: rnn_amd_set_multi_calc_deltas before any multi-head loss\n");
    abort();
  }
  /* (heads of at least 24 columns: a stream's ranges then lie at least 16 columns apart, see k_top_backprop_heads) */
  ramd_set_calc_deltas(set, accumulate, NULL, NULL, NULL, e->mheads_alen >= 24 ? RAMD_RANGES_ARE_HEADS : 0,
                       e->d_mranges + (size_t)set->row0 * MULTI_RANGE_STRIDE, MULTI_RANGE_STRIDE, defer);
}
void rnn_amd_set_multi_calc_deltas(RnnAmdSet *set, int accumulate) { multi_calc_deltas(set, accumulate, NULL); }

/* The multi-head step's offer to generate the next pass's noise between its forward pass and its loss of `classes` heads
 * (noise_ahead.c): made where the pass has its seam -- from the fused hidden layer's end on, beside the output layer and
 * the loss -- or else right behind the pass, and only when the pass took its own noise from a slot.  offered: it has been
 * made, so the loss makes none of its own. */
typedef struct EarlyOffer {
  RnnAmdSet *set;
  int classes, offered;
} EarlyOffer;

static void early_offer(void *ctx) {
  EarlyOffer *o = ctx;
  if (!o->offered && ramd_noise_ahead_adopted(o->set->eng)) {
    ramd_noise_ahead_offer(o->set, o->classes);
    o->offered = 1;
  }
}

void ramd_set_multi_step_deltas(RnnAmdSet *set, const int *hot, const int *next, const int *target_class, int alphabet_len,
                                float leakage, int accumulate, RamdPendingDelta *defer) {
  RamdEngine *e = set->eng;
  ramd_set_need_training(set, "rnn_amd_set_multi_step_deltas");
  int n_classes = multi_heads(e, alphabet_len);
  /* the three small uploads leave with one launch */
  ramd_upload_q(e->b.hot + set->row0, hot, set->n * sizeof(int));
  if (target_class) {
    ramd_upload_q(e->d_mclass + set->row0, target_class, set->n * sizeof(int));
    noise_ahead_classes(&e->ahead, target_class, set->n, n_classes);
  }
  ramd_upload(e->b.target + set->row0, next, set->n * sizeof(int));
  EarlyOffer early = {set, n_classes, 0};
  ramd_set_forward_seam(set, RAMD_IN_ONE_HOT, NULL, 0, 0, NULL, 1, RAMD_FWD_WHOLE, early_offer, &early);
  early_offer(&early); /* (a pass without the seam) */
  multi_loss(set, NULL, alphabet_len, n_classes, leakage, early.offered);
  multi_calc_deltas(set, accumulate, defer);
}
void rnn_amd_set_multi_step_deltas(RnnAmdSet *set, const int *hot, const int *next,
                                   const int *target_class, int alphabet_len, float leakage,
                                   int accumulate) {
  ramd_set_multi_step_deltas(set, hot, next, target_class, alphabet_len, leakage, accumulate, NULL);
}

/* the same from the text on the device: stream j reads text[o] and is scored against
 * text[o + 1], o as in rnn_amd_set_char_step */
void rnn_amd_set_multi_text_loss(RnnAmdSet *set, int i, const int *target_class, int alphabet_len,
                                 float leakage) {
  RamdEngine *e = set->eng;
  ramd_set_need_training(set, "rnn_amd_set_multi_text_loss");
  ramd_set_check_text_pos(e, i, 0, "rnn_amd_set_multi_text_loss");
  int n_classes = multi_heads(e, alphabet_len);
  ramd_set_forward(set, RAMD_IN_TEXT, NULL, 0, i, NULL, 1, RAMD_FWD_WHOLE); /* advance + one-hot opinion + b.target */
  multi_loss(set, target_class, alphabet_len, n_classes, leakage, 0);
}

/* ---- the dense losses ----
 * rnnca's (gstrnnca.c:701-714; sigmoid_rule.h): sigmoid of the first n outputs in place, o_error = slope * (target - answer);
 * the row's squared error and a count go into the set's statistics only with `stats` -- rnn_amd_set_automaton_steps alone
 * asks for that, the public calls leave the statistics alone.  Parrot's (train_net, gstparrot.c:464-477; parrot_rule.h):
 * tanh in place, (1 - a a) (target - a), the statistics always.  targets: host [n_nets][ld], or (on_dev) device rows ld
 * floats apart: a block trainer's. */

void ramd_set_dense_loss_check(const RnnAmdSet *set, RamdDenseLoss kind, const char *what, const float *targets, int ld,
                               int n) {
  ramd_set_need_training(set, what);
  const int outputs = set->eng->sh.output_size;
  const int parrot = kind == RAMD_DENSE_TANH_SLOPE;
  if ((parrot && !targets) || n < 1 || n > outputs || ld < n) {
    if (parrot) {
      fprintf(stderr, "librecur_amd: %s: targets %p over %d of %d outputs (ld %d)\n", what, (const void *)targets, n, outputs, ld);
    } else {
      fprintf(stderr, "librecur_amd: %s over %d of %d outputs (ld %d)\n", what, n, outputs, ld);
    }
    abort();
  }
}

/* The targets are the caller's host rows: room for them in d_group and the rows on their way there -- at once, or with
 * `inputs` queued behind the call's dense input rows, so that both leave with the ring indices in the flush of the pass
 * that is still to come.  -> the device rows, n floats apart */
static const float *dense_targets_stage(RnnAmdSet *set, const float *inputs, int ld_inputs, const float *targets, int ld,
                                        int n) {
  RamdEngine *e = set->eng;
  group_room(e, (size_t)set->n * n * sizeof(float));
  if (inputs) {
    ramd_upload_rows_q(e->d_dense, inputs, ld_inputs * sizeof(float), e->sh.input_size * sizeof(float), set->n, 0);
  }
  ramd_upload_rows_q(e->d_group, targets, ld * sizeof(float), n * sizeof(float), set->n, inputs == NULL);
  return (const float *)e->d_group;
}

/* the loss behind a finished pass */
static void set_dense_loss(RnnAmdSet *set, RamdDenseLoss kind, const float *targets, int ld, int n, int on_dev, int stats) {
  RamdEngine *e = set->eng;
  ramd_top_done_clear(e);
  ramd_set_streams_to_dev(set);
  if (!on_dev) {
    targets = dense_targets_stage(set, NULL, 0, targets, ld, n);
    ld = n;
  }
  ramd_launch_dense_loss(ramd_stream, &e->sh, &e->b, set->row0, set->n, kind, n, targets, ld, stats);
  ramd_set_streams_dev_wrote(set);
}

void rnn_amd_set_sigmoid_mse_error(RnnAmdSet *set, const float *targets, int ld, int n) {
  ramd_set_dense_loss_check(set, RAMD_DENSE_SIGMOID_MSE, "rnn_amd_set_sigmoid_mse_error", targets, ld, n);
  set_dense_loss(set, RAMD_DENSE_SIGMOID_MSE, targets, ld, n, 0, 0);
}

void rnn_amd_set_tanh_error(RnnAmdSet *set, const float *targets, int ld, int n) {
  ramd_set_dense_loss_check(set, RAMD_DENSE_TANH_SLOPE, "rnn_amd_set_tanh_error", targets, ld, n);
  set_dense_loss(set, RAMD_DENSE_TANH_SLOPE, targets, ld, n, 0, 0);
}

/* (on_dev never comes with a bottom layer: rnn_amd_set_automaton_steps refuses such a set, rnn_amd_set_dense_steps_tanh
 * keeps its frames on the host) */
void ramd_set_opinion_dense_loss(RnnAmdSet *set, RamdDenseLoss kind, const float *inputs, int ld_inputs, const float *targets,
                                 int ld, int n, int on_dev, int advance, int stats) {
  RamdEngine *e = set->eng;
  if (!ramd_set_dense_top_ok(set, inputs, kind)) {
    if (on_dev) {
      ramd_set_forward(set, RAMD_IN_DENSE, inputs, ld_inputs, 0, NULL, advance, RAMD_FWD_WHOLE);
    } else {
      if (advance) {
        rnn_amd_set_advance(set);
      }
      rnn_amd_set_opinion(set, inputs, ld_inputs, NULL);
    }
    set_dense_loss(set, kind, targets, ld, n, on_dev, stats);
    return;
  }
  if (!on_dev) {
    targets = dense_targets_stage(set, inputs, ld_inputs, targets, ld, n);
    ld = n;
    inputs = e->d_dense;
    ld_inputs = e->sh.input_size;
  }
  const RamdHandover left = ramd_set_forward(set, RAMD_IN_DENSE, inputs, ld_inputs, 0, NULL, advance, RAMD_FWD_FOR_DENSE_TOP);
  const RamdTopLoss loss = {.kind = kind, .targets = targets, .ld = ld, .n = n, .stats = stats};
  if (!ramd_launch_dense_top(ramd_stream, &e->sh, &e->b, set->row0, set->n, left, &loss)) {
    fprintf(stderr, "librecur_amd: %s: the top launch declined a shape it had accepted\n",
            kind == RAMD_DENSE_TANH_SLOPE ? "rnn_amd_set_opinion_tanh_error" : "rnn_amd_set_opinion_sigmoid_mse");
    abort();
  }
  ramd_set_streams_dev_wrote(set);
  ramd_top_done_set(e, set->row0, set->n, 0);
}

/* (the check names rnn_amd_set_sigmoid_mse_error: the call has always left its refusals to that one) */
void rnn_amd_set_opinion_sigmoid_mse(RnnAmdSet *set, const float *inputs, int ld_inputs, const float *targets, int ld,
                                     int n) {
  ramd_set_dense_loss_check(set, RAMD_DENSE_SIGMOID_MSE, "rnn_amd_set_sigmoid_mse_error", targets, ld, n);
  ramd_set_opinion_dense_loss(set, RAMD_DENSE_SIGMOID_MSE, inputs, ld_inputs, targets, ld, n, 0, 0, 0);
}

void rnn_amd_set_opinion_tanh_error(RnnAmdSet *set, const float *inputs, int ld_inputs, const float *targets, int ld,
                                    int n) {
  ramd_set_dense_loss_check(set, RAMD_DENSE_TANH_SLOPE, "rnn_amd_set_opinion_tanh_error", targets, ld, n);
  ramd_set_opinion_dense_loss(set, RAMD_DENSE_TANH_SLOPE, inputs, ld_inputs, targets, ld, n, 0, 0, 0);
}
