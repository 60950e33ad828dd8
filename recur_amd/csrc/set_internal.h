/* set_internal.h -- what the three files of the batched API share among themselves (gnu11 C):
 *   set_api.c    the set's lifecycle and sharding, the forward pass and the opinion calls, the delta call
 *   set_loss.c   what lies between a pass and its delta call: every loss, and the opinion-plus-loss forms
 *   set_train.c  whole generations: the one-call steps (set_step) and the three block trainers
 * Each function stands in the file named above its declaration; what only one file uses is static there.
 * (ramd_set_need_training is rnn_host.h's: noise_ahead.c and exchange.c ask it too.) */
#ifndef RAMD_SET_INTERNAL_H
#define RAMD_SET_INTERNAL_H 1
#include "rnn_host.h"

/* the dense losses: a target row per stream against the first n outputs; the values are the top launch's kinds */
typedef enum RamdDenseLoss {
  RAMD_DENSE_SIGMOID_MSE = RAMD_TOP_SIGMOID_MSE, /* rnnca's (gstrnnca.c:701-714, sigmoid_rule.h) */
  RAMD_DENSE_TANH_SLOPE = RAMD_TOP_TANH_SLOPE    /* parrot's (gstparrot.c:464-477, parrot_rule.h) */
} RamdDenseLoss;

/* ---- set_api.c ---- */
/* the streams' state is current on the device (and their ring indices pushed) / the device has just written it */
void ramd_set_streams_to_dev(RnnAmdSet *set);
void ramd_set_streams_dev_wrote(RnnAmdSet *set);
/* The set's forward pass.  want (RAMD_FWD_*): the whole pass, or stop after the hidden layer's sums and leave them for
 * ramd_launch_text_top / ramd_launch_dense_top; returns what was left (nothing otherwise).  seam (or NULL): called with ctx
 * at the pass's seam where it has one (ramd_launch_forward) */
RamdHandover ramd_set_forward_seam(RnnAmdSet *set, int mode, const float *d_dense, int ld, int text_i, float *outputs,
                                   int advance, int want, void (*seam)(void *ctx), void *ctx);
static inline RamdHandover ramd_set_forward(RnnAmdSet *set, int mode, const float *d_dense, int ld, int text_i,
                                            float *outputs, int advance, int want) {
  return ramd_set_forward_seam(set, mode, d_dense, ld, text_i, outputs, advance, want, NULL, NULL);
}
/* the set calls' active mask on the device (b.active), uploaded unless these very flags are there already; queued: leaves
 * with the caller's next flush */
void ramd_set_active_mask_to_dev(RamdEngine *e, const u8 *active, int n, int queued);
/* rnn_amd_set_calc_deltas with everything its internal callers add: see the definition */
void ramd_set_calc_deltas(RnnAmdSet *set, int accumulate, RecurErrorRange *ranges, const u8 *active, const u8 *dev_active,
                          unsigned extra_flags, const int *dev_ranges, int range_stride, RamdPendingDelta *defer);
/* a text is loaded and position i lies in [0, text_len - 1 + last_ok), or the call `what` aborts */
void ramd_set_check_text_pos(RamdEngine *e, int i, int last_ok, const char *what);

/* ---- set_loss.c ---- */
/* what a public call of a dense loss checks once, up front (the forms below take checked arguments): a training set,
 * 1 <= n <= output_size and rows of at least n floats; parrot's calls refuse NULL targets too.  `what` names the call in
 * the message */
void ramd_set_dense_loss_check(const RnnAmdSet *set, RamdDenseLoss kind, const char *what, const float *targets, int ld,
                               int n);
/* the forward pass of dense input rows with a dense loss behind it, as one top launch where that takes the set (the delta
 * call that follows then skips the top layer's backprop) and as pass + loss elsewhere.  on_dev: inputs and targets are
 * device rows, ld_inputs and ld floats apart (a block trainer's); else the caller's host rows.  advance: rnn_bptt_advance
 * first.  stats: rnnca's loss adds to the set's statistics (parrot's always does) */
void ramd_set_opinion_dense_loss(RnnAmdSet *set, RamdDenseLoss kind, const float *inputs, int ld_inputs, const float *targets,
                                 int ld, int n, int on_dev, int advance, int stats);
/* whether the class-group top launch can follow a pass of these dense inputs, and that pass and launch for rows already on
 * the device: see the definitions */
int ramd_set_dense_top_ok(RnnAmdSet *set, const float *inputs, int kind);
void ramd_set_class_group_top(RnnAmdSet *set, const char *what, const float *d_inputs, int ld_inputs, int advance,
                              const RamdTopLoss *groups, const u8 *trained);
/* rnn_amd_set_multi_step_deltas with the delta call's `defer` */
void ramd_set_multi_step_deltas(RnnAmdSet *set, const int *hot, const int *next, const int *target_class, int alphabet_len,
                                float leakage, int accumulate, RamdPendingDelta *defer);

#endif
