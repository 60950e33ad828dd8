/* ramd_internal.h -- private interface between the gnu11 C host code
 * (engine.c, net_api.c, set_api.c, set_loss.c, set_train.c, noise_ahead.c, exchange.c, rnn_init.c, rnn_io.c) and the
 * HIP kernels and their launchers (kernels_*.hip).
 *
 * The C side owns residency, coherence and call order: what lives where, when
 * to copy, which ramd_launch_* follows which.  The launchers own the choice of
 * kernel form for a shape: a ramd_launch_* function enqueues on the given
 * stream whichever of its kernels (one, or a short sequence) suits the sizes,
 * the flags and the RECUR_AMD_* switches, and returns.
 */
#ifndef RAMD_INTERNAL_H
#define RAMD_INTERNAL_H 1
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Shape of one engine: a set of weights and the streams that share it. */
typedef struct RamdShape {
  int input_size, hidden_size, output_size;
  int I, H, O;    /* padded sizes (multiples of 4), recur-nn-init.c:87-91 */
  int D;          /* BPTT ring depth                                      */
  int Scap;       /* capacity in training streams: row stride of a slot    */
  int Fcap;       /* capacity in forward-only streams                      */
  int activation; /* rnn_activation                                        */
  /* optional bottom layer (recur-nn.h:211-227): b_in real inputs (+ bias) feed
   * b_out = input_size rectified outputs; bI, bO are its padded sizes, 0 without one */
  int b_in, b_out, bI, bO;
} RamdShape;
/* row length of RamdBuffers::ex: column 0 and the columns above hidden_size (the real inputs and the pad), whole float4s */
static inline int ramd_nxp(const RamdShape *sh) { return (sh->I - sh->hidden_size + 3) & ~3; }

/* Device arrays.  "state row" r addresses hidden/out: r < Scap is training
 * stream r, r >= Scap is forward-only stream r - Scap.
 *
 * HBM layout (all fp32, row major):
 *   arena   [D][Scap][I] history ring, slot major, then [Fcap][I] input rows
 *           of the forward-only streams
 *   ehi     [D+1][Scap][I] back-propagated error per BPTT step (columns
 *           1..hidden_size; column 0 and the columns above stay zero): row 0 is the
 *           (soft-clipped) top-layer error, row t+1 the input error of step t
 *   esum    [D][Scap]  sum of squares of each step's input error
 *   coef    [D][Scap]  ih_scale of the stream while the step was executed, else 0
 */
typedef struct RamdBuffers {
  float *ih_w, *ho_w, *ih_m, *ho_m, *ih_aux, *ho_aux, *ih_delta, *ho_delta;
  float *arena, *hidden, *out, *o_error, *err_a, *err_b, *ehi, *esum, *coef;
  float *ex;        /* [D+1][Scap][nxp] column 0 and the input columns of each step's error */
  float *esum_part; /* [D][tn+1][Scap] per-column-tile partial sums of squares         */
  float *zeros;     /* 256 bytes of zeros: source of out-of-range LDS-DMA chunks       */
  unsigned long long *rng; /* [Scap+Fcap][4] each stream's generator (recur-rng.h:15-20)   */
  float *ones;      /* [Scap] of 1.0: the "every stream takes part" mask               */
  float *slab;
  float *ho_slab; /* 8 planes of H * O for the deferred top-layer delta sum, or NULL (very wide O) */
  size_t slab_floats;
  int *idx;       /* [Scap] ring position                           */
  float *lr;      /* [Scap] each stream's own learn_rate copy        */
  float *mef;     /* [Scap] min_error_factor                         */
  float *ih_scale, *top_raw, *top_scaled, *bptt_err; /* [Scap]       */
  int *n_exec;    /* [Scap] executed BPTT steps                      */
  int *depth_log; /* [Scap] "depth - t" as the reference logs it     */
  int *target;    /* [Scap+Fcap] class the loss kernels score against */
  double *xent;   /* [Scap+Fcap] running sum of log2 p(target), k_xent_accumulate */
  int *hot;       /* [Scap+Fcap] one-hot input index scratch         */
  unsigned char *active; /* [Scap] scratch for the active mask       */
  /* per-stream loss statistics (single writer per entry: deterministic) */
  double *stat_err, *stat_ent, *stat_zero, *stat_depth; /* [Scap]    */
  long long *stat_correct, *stat_count;                 /* [Scap]    */
  unsigned char *text;   /* encoded text for the host-free epoch loop */
  int text_len;
  /* bottom layer: weights and their optimiser arrays [bI][bO]; each stream's input row
   * binp [Scap+Fcap][bI] and raw output row bout [Scap+Fcap][bO]; berr [Scap][bO] the
   * stream's input error summed over its executed BPTT steps; bcarry [2][bO] the
   * reference's never-cleared bottom->o_error accumulator (ping-pong, bcarry_cur = the
   * current one) */
  float *bw, *bm, *baux, *bdelta, *binp, *bout, *berr, *bcarry;
  /* the layer has ONE input buffer for all clones and one_hot_opinion never clears its last entry
   * (charmodel-helpers.h:20-31): that entry, as the last dense / kept forward pass left it */
  float *blast;
  int bcarry_cur;
  /* ring position shared by every training stream of the current call, or -1
   * when they differ (set by the host before each launch) */
  int uniform_idx;
  /* presynaptic noise generated ahead of its forward pass (noise_ahead.c, which sets these for one
   * pass and clears them behind it): [n][H] values and the generator states after them;
   * noise_spec_use: the next forward adds these and adopts the states instead of running the generators */
  float *noise_spec;
  void *rng_spec;
  int noise_spec_use;
  /* hint: the set's last forward pass took dense input rows (audio features, pixels) rather than
   * one-hot symbols -- the extras of the BPTT chain are then a GEMM, not a gather over the few
   * non-zero input rows (either is correct for any input) */
  int dense_inputs;
  /* symbols per head of the last multi-head loss on these rows (0: none): with RAMD_RANGES_ARE_HEADS the range lists
   * are runs of whole heads of this many columns */
  int mheads_alen;
  /* [Scap][heads][H] partial products of the sparse top backprop (k_top_heads_partial), or NULL */
  float *mheads_part;
  size_t mheads_part_floats;
} RamdBuffers;

/* ih_delta left as un-summed K slabs by ramd_launch_calc_deltas, for the optimiser launch
 * that follows immediately to sum (and store) itself; slab == NULL: nothing pending */
typedef struct RamdPendingDelta {
  const float *slab;   /* [ks][n] planes of the rows below rows_core                  */
  size_t n;            /* plane stride = I * H                                        */
  int ks, H, hidden_size, rows_core, ks_rest;
  const float *rest;   /* planes of the rows from rows_core on: rest + z * rest_stride */
  size_t rest_stride;
  float *delta_out;    /* ih_delta                                                    */
  /* the same for ho_delta (the top layer's GEMM keeps its slabs in b->ho_slab, which nothing
   * else uses); ho_slab == NULL: ho_delta has been summed already */
  const float *ho_slab;
  size_t ho_n;         /* plane stride = H * O */
  int ho_ks;
  float *ho_delta_out;
  /* in: a workspace of the caller's own for the planes (own_slab_floats of it) instead of the shared split-K
   * workspace -- for sums that are to outlive the call (the engine's kept deltas, set_api.c) */
  float *own_slab;
  size_t own_slab_floats;
  /* in: the update that follows, should the weight-delta GEMM be able to carry it out itself (k_delta_direct's
   * epilogue + k_apply_edges: rnn_apply_learning's momentum rule, recur-nn.c:482-487, with these rates) --
   * fuse_want != 0 asks; out: fuse_done != 0 says that weights and momentum ARE updated (both layers) and the
   * delta arrays hold the sums: nothing is left pending */
  int fuse_want, fuse_done;
  float fuse_rate, fuse_ho_rate, fuse_momentum, fuse_mw;
  int fuse_method; /* 0: the momentum rule (recur-nn.c:482-487); 4: ADAGRAD (recur-nn.c:518-524; round 6) */
} RamdPendingDelta;

enum { RAMD_IN_KEEP = 0, RAMD_IN_ONE_HOT = 1, RAMD_IN_DENSE = 2, RAMD_IN_TEXT = 3 };

typedef void *ramd_stream_t;

/* sums what ramd_launch_calc_deltas left pending into the delta arrays after all (nobody took it along) */
void ramd_launch_pending_finalize(ramd_stream_t st, const RamdPendingDelta *p);

/* ---- forward ---- */
/* What a caller wants of a forward pass (rnn_opinion, recur-nn.c:83-154).  The real inputs of state rows
 * [row0, row0 + nrows) come as `mode` says: dense is a device pointer with leading dimension ld; text_i is the text
 * position for RAMD_IN_TEXT (also fills b->target); the row's global stream number is global_first + (row - row0) of
 * global_count.  With a bottom layer (recur-nn.c:88-103) the inputs feed that layer, whose rectified outputs become
 * the real inputs. */
enum {
  RAMD_FWD_WHOLE = 0,         /* hidden = act(X . W_ih), out = hidden . W_ho (recur-nn.c:117-151) */
  RAMD_FWD_FOR_TEXT_TOP = 1,  /* the hidden layer's sums stay in the workspace for ramd_launch_text_top */
  RAMD_FWD_FOR_DENSE_TOP = 2  /* ... for ramd_launch_dense_top */
};
typedef struct RamdFwdCall {
  int row0, nrows, mode;
  const float *dense;
  int ld, text_i, global_first, global_count;
  int advance;     /* step each stream's ring index first (rnn_bptt_advance) */
  float noise;     /* presynaptic_noise */
  int fwd_only;    /* forward-only rows (above Scap) */
  int want;        /* RAMD_FWD_* */
  int rows_built;  /* the input rows are there already (ramd_launch_texts_step built them) */
  int one_net;     /* rnn_opinion for one net: the one-launch form for small nets may take it */
} RamdFwdCall;
/* What a pass that stops for a top launch leaves in the workspace: `planes` K slabs of the hidden layer's sums
 * (0: nothing), or one plane and `partials` per-tile partial sums of the h_size padding columns behind it.  top_done: a
 * pass for the text step's top launch has run that top layer in its own launch (fwd_top_plan.h): nothing is left, and
 * ramd_launch_text_top is not to follow */
typedef struct RamdHandover {
  int planes, partials;
  int top_done;
} RamdHandover;
/* The pass: fwd_plan.h says which kernels, this enqueues them.  `seam` (or NULL) is called with `ctx` between the
 * hidden layer's end and the output layer where the hidden layer was the fused launch with its own finishing kernel,
 * and nowhere else (set_loss.c: the multi-head step offers the next pass's noise to noise_ahead.c there). */
RamdHandover ramd_launch_forward(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b, const RamdFwdCall *call,
                                 void (*seam)(void *ctx), void *ctx);
/* the bottom layer's share of rnn_bptt_calc_deltas (recur-nn.c:377-382, 750-757) for
 * rows that ramd_launch_calc_deltas has just processed; flips b->bcarry_cur */
void ramd_launch_bottom_deltas(ramd_stream_t st, const RamdShape *sh, RamdBuffers *b, int row0,
                               int nrows, int accumulate, const unsigned char *active);
/* output layer + softmax error against b->target + dense top backprop in one launch (what
 * the forward pass's output layer, ramd_launch_softmax_error and the first kernel of
 * ramd_launch_calc_deltas do); follow with ramd_launch_calc_deltas(flags | RAMD_TOP_DONE).
 * ramd_text_top_ok says whether the shape allows it. */
#define RAMD_TOP_DONE 0x40000000u
/* flag of ramd_launch_calc_deltas: the per-stream range lists are the multi-head loss's (runs of whole heads of at
 * least 24 columns, the error row zero outside them): the top backprop may run as one GEMM (k_top_backprop_heads) */
#define RAMD_RANGES_ARE_HEADS 0x10000000u
/* flag of ramd_launch_calc_deltas: the error images (err_a / err_b) of these very rows have not been rebuilt since
 * their last BPTT run (k_err_writeback pending).  The ranged top backprops keep the images' stale entries for rows
 * whose hidden value is zero: the launcher rebuilds the images first, unless its top-layer form
 * takes the stale entries from the error planes itself (k_top_heads_combine) */
#define RAMD_IMAGES_PENDING 0x08000000u
/* flag of ramd_launch_calc_deltas: the fused single-net path (rnn_bptt_calculate): no ho_delta is formed, the top
 * layer's weights are updated directly by the ramd_launch_fused_updates that follows */
#define RAMD_NO_HO_DELTA 0x80000000u
/* flag of ramd_launch_calc_deltas: that path unbatched: ih_delta gets the UNSCALED sum, the stream's ih_scale goes
 * into the rate of the update, not into the sum (recur-nn.c:966-975) */
#define RAMD_IH_SCALE_IN_RATE 0x20000000u
/* a stream's range list as the multi-head loss leaves it: up to 64 + 1 (start, len) pairs, then one bit per head the
 * stream trained (an unsigned long long at this int offset; the stride keeps it 8-byte aligned) */
#define RAMD_HEADBITS_AT 130
#define RAMD_MULTI_RANGE_STRIDE 132
int ramd_text_top_ok(const RamdShape *sh);
void ramd_launch_text_top(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b, int row0,
                          int nrows, RamdHandover left);
/* The same launch with another loss between the output layer and the backprop, handed one struct as the batched rows'
 * launches below are: the host fills it, the launcher checks it, the kernel (k_text_top<kind>) takes it by value.
 *   RAMD_TOP_SIGMOID_MSE   rnnca's loss (sigmoid_rule.h): targets [nrows][ld] on the device, the first n outputs.  stats
 *                          (rnn_amd_set_automaton_steps alone): the row's sum of (target - a)^2 and one count into the
 *                          statistics
 *   RAMD_TOP_CLASS_GROUPS  gstclassify's class groups: offsets, sizes, targets gt [nrows][ngroups], per-output weights or
 *                          NULL.  gate (rnn_amd_set_classify_steps alone; or NULL): a device word that a trained row whose
 *                          summed wrongness is not 0.0f sets to 1 (classify_train_rule.h)
 *   RAMD_TOP_TANH_SLOPE    parrot's loss (parrot_rule.h): targets as rnnca's; tanh in place on the first n outputs, (1 - a a)
 *                          (target - a), the row's squared error into the statistics
 * stats and gate are ignored for the kinds that do not own them.  ramd_dense_top_ok(sh, kind): the launch will take the shape
 * (the text top's; O <= 64 for the one-wave kinds 1 and 2; the RECUR_AMD_DENSE_TOP switch); the launch returns 0 where it
 * does not, and nothing was launched. */
enum { RAMD_TOP_TEXT = 0, RAMD_TOP_SIGMOID_MSE = 1, RAMD_TOP_CLASS_GROUPS = 2, RAMD_TOP_TANH_SLOPE = 3 };
typedef struct RamdTopLoss {
  const float *targets; /* 1, 3: [nrows][ld] */
  int ld, n;
  int ngroups;          /* 2 */
  const int *goff, *gsize, *gt;
  const float *weight;
  int stats;            /* 1 */
  int kind;             /* RAMD_TOP_* */
  unsigned *gate;       /* 2 */
} RamdTopLoss;
int ramd_dense_top_ok(const RamdShape *sh, int kind);
int ramd_launch_dense_top(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b, int row0, int nrows, RamdHandover left,
                          const RamdTopLoss *loss);
/* o_error = onehot(target) - softmax(out) and statistics
 * (charmodel-predict.c:18-27, 299-304) */
void ramd_launch_softmax_error(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b,
                               int row0, int nrows);

/* one step of get_cross_entropy (charmodel-predict.c:71-76) for state row `row`: adds
 * capped_log2f(softmax(out)[target]) to b->xent[row] when count_it */
void ramd_launch_xent_accumulate(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b,
                                 int row, int count_it);

/* ---- backward ---- */
/* ranges: device array of (start,len) pairs ending with start < 0, or NULL;
 * active: device mask per row or NULL.  accumulate == 0 zeroes the deltas
 * first.  This is rnn_bptt_calc_deltas (recur-nn.c:707-772) for the rows. */
void ramd_launch_calc_deltas(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b,
                             int row0, int nrows, int accumulate, const int *ranges,
                             int range_stride, const unsigned char *active, unsigned flags,
                             RamdPendingDelta *defer);
/* train_channel's loss (gstclassify.c:2070-2119): softmax error per class group against
 * gt[row][group] (< 0: the group is not trained), then the per-output error weights; all
 * arrays are device pointers, `largest` the largest group size; gate (or NULL): as ramd_launch_dense_top's */
void ramd_launch_grouped_softmax_error(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b,
                                       int row0, int nrows, int ngroups, int largest,
                                       const int *goff, const int *gsize, const int *gt,
                                       const float *weight, unsigned *gate);
/* multi_softmax_error (charmodel-multi-predict.c:17-58) for rows whose opinion has been
 * formed: b->target holds each stream's next symbol, tclass[j] its own class head;
 * writes o_error and, per stream, the merged (start, len) range list (terminated by
 * start < 0) at ranges + j * range_stride */
void ramd_launch_multi_softmax_error(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b,
                                     int row0, int nrows, int alphabet_len, int n_classes,
                                     unsigned long long threshold, const int *tclass, int *ranges,
                                     int range_stride);
/* one step of rnn_char_multi_cross_entropy (charmodel-multi-predict.c:395-403) for state row
 * `row`: per head c, capped log2 of softmax(head c)[target] added to acc[c] (device doubles) */
void ramd_launch_multi_xent_accumulate(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b,
                                       int row, int alphabet_len, int n_classes, double *acc,
                                       int count_it);
/* ---- the batched forward-only calls (kernels_rows.hip) ----
 * Each call has ONE launch between two forward passes of its rows, and each launch is handed one struct: the host fills it
 * once per wave or segment and sets what changes per launch; the launcher checks it and the kernel takes it by value (the
 * text scorer's: the fields of its form).  In all of them row0 is the state row of the wave's row 0, a forward-only row (texts_plan.h's order: the rows still running
 * are a prefix), hid0 the hidden row every row's FIRST feed is built on -- NULL: on the row's own hidden values, as every
 * later feed is (the caller has put the rows' start states there) --, and every pointer a device pointer. */

/* rnn_amd_run_texts and rnn_amd_trace_texts (texts_api.c): N texts of different lengths through one net.  Two halves:
 *   score step t_score, rows [0, a_score): what k_xent_accumulate / k_multi_xent_accumulate do -- softmax of the output
 *     row (n_sums == 1), or of each of its n_sums heads of alen outputs (badmaths.h:71-111, the sum in the reference's
 *     order), capped log2 of the probability of text[t_score + 1].  The sums form (trace == NULL) adds the float to
 *     acc[row][n_sums], leaving out the rows with skip[row] > t_score.  The trace form has no skip: it stores the float at
 *     trace[off_tr[row] + t_score * n_sums + head] and, with guess != NULL, the head's best guess (softmax_best_guess: the
 *     largest likelihood, the lowest index among equals) as a byte at the same index of guess.  Row j is traced at every
 *     t < len_j - 1, so every entry has one writer and is written once; nothing else of either array is touched.
 *   feed step t_feed, rows [0, a_feed): the input row of the next forward pass -- the one-hot of text[t_feed]
 *     (charmodel-helpers.h:16-33) on the hidden values.
 * a_score == 0: a wave's first launch, which only feeds; a_feed == 0: its last, which only scores. */
typedef struct RamdTextsStep {
  const unsigned char *text;        /* the wave's texts behind one another            */
  const unsigned long long *off;    /* [rows] where row j's text starts               */
  const int *skip;                  /* sums: [rows] steps fed but not scored          */
  double *acc;                      /* sums: [rows][n_sums] running sums              */
  const unsigned long long *off_tr; /* trace: [rows] where row j's trace starts, in entries */
  float *trace;                     /* trace: the wave's log2 likelihoods, or NULL: the sums form */
  unsigned char *guess;             /* trace: the wave's best guesses, or NULL        */
  const float *hid0;
  int row0;
  int alen, n_sums;
  int t_score, a_score, t_feed, a_feed;
} RamdTextsStep;
void ramd_launch_texts_step(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b, const RamdTextsStep *p);

/* rnn_amd_run_sequences (seqs_api.c): a wave of dense feature sequences and one segment of their frames, staged behind
 * one another (seqs_plan.h: row j's frame i at in[(off[j] + i) * input_size], its answers at ans[(off[j] + i) *
 * output_size], its winners at win[(off[j] + i) * n_groups]; t_score and t_feed count within the segment).  Two halves:
 *   score frame t_score, rows [0, a_score): the softmax probability within its group for a column of one of the n_groups
 *     class groups, the raw output for the n_gap columns in no group (with no groups every column), and with win != NULL
 *     softmax_best_guess's pick per group as a byte.  Every entry has one writer and is written once.
 *   feed frame t_feed, rows [0, a_feed): the input row of the next forward pass from the staged frame.
 * a_score == 0: the first launch of a segment, which only feeds; a_feed == 0: its last, which only scores. */
typedef struct RamdSeqsStep {
  const float *in;               /* the segment's staged frames                    */
  float *ans;                    /* the segment's answers                          */
  unsigned char *win;            /* the segment's winners, or NULL                 */
  const unsigned long long *off; /* [rows] where row j's frames start, in frames   */
  const int *goff, *gsize;       /* [n_groups] the class groups                    */
  const int *gap;                /* [n_gap] the columns in no group, ascending     */
  const float *hid0;
  int row0;
  int n_groups, n_gap;
  union {
    int largest;                 /* the host's: the largest group's size                                     */
    int stride;                  /* the kernel's: a wave's floats of LDS, which the launcher writes over it in its own copy */
  };
  int t_score, a_score, t_feed, a_feed;
} RamdSeqsStep;
void ramd_launch_seqs_step(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b, const RamdSeqsStep *p);

/* rnn_amd_classify_texts (classify_texts_api.c): N texts of different lengths through one classifier net, every symbol fed
 * AND scored (the plan's text of len + 1: len forward passes, as the sequences').  Two halves:
 *   score symbol t_score, rows [0, a_score) whose skip[row] <= t_score (classify_rule.h): the softmax of the row's
 *     output_size outputs as ONE group (badmaths.h:71-111: the shift, fast_expf, the sum in index order, the division).
 *     Row j's accumulators are RAMD_CLASSIFY_ACC_WORDS(output_size) 8-byte words at acc + j * that: output_size doubles
 *     that p[c] is added to, output_size doubles that the float product p[c] * p[c] is added to, then -- for a symbol
 *     whose class byte cl = cls[off[row] + t_score] is not 0xFF (cls NULL: no symbol has a class) -- a double that
 *     1 - p[cl] is added to, a double that capped_log2f(p[cl]) is subtracted from, and two long longs: one counts the
 *     symbols whose best guess (softmax_best_guess: the largest probability, the lowest index among equals) is cl, one
 *     the symbols with a class.  The host zeroes them per wave; every word has one writer: no atomics.
 *   feed symbol t_feed, rows [0, a_feed): the input row of the next forward pass -- the one-hot of text[t_feed] on the
 *     hidden values.
 * a_score == 0: a wave's first launch, which only feeds; a_feed == 0: its last, which only scores. */
#define RAMD_CLASSIFY_ACC_WORDS(output_size) (2 * (size_t)(output_size) + 4)
typedef struct RamdClassifyStep {
  const unsigned char *text;     /* the wave's texts behind one another            */
  const unsigned char *cls;      /* their class bytes at the same offsets, or NULL */
  const unsigned long long *off; /* [rows] where row j's text starts               */
  const int *skip;               /* [rows] symbols fed but not scored              */
  double *acc;                   /* [rows][RAMD_CLASSIFY_ACC_WORDS] (above)        */
  const float *hid0;
  int row0;
  int t_score, a_score, t_feed, a_feed;
} RamdClassifyStep;
void ramd_launch_classify_step(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b, const RamdClassifyStep *p);

/* rnn_amd_run_automaton (automaton_api.c): RamdAutomatonStep stands in automaton_rule.h, next to the rule it embeds */
struct RamdAutomatonStep;
void ramd_launch_automaton_step(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b,
                                const struct RamdAutomatonStep *p);
/* rnn_amd_set_automaton_steps (set_train.c): the one gather launch of a block (kernels_automaton_train.hip).
 * RamdAutomatonTrainRows and its contract stand in automaton_train_rule.h, next to the rule it embeds */
struct RamdAutomatonTrainRows;
void ramd_launch_automaton_train_rows(ramd_stream_t st, const struct RamdAutomatonTrainRows *p);

/* rnn_amd_dream_sequences (dream_api.c): parrot's player (fill_audio_chunk, gstparrot.c:556-583) for `rows` sequences in
 * lock step, sequence k on forward-only state row row0 + k, each fed its own last answer; the net has as many inputs as
 * outputs.  The rule is dream_rule.h's.  Three kinds of launch:
 *   a call's first (first != NULL): the input row of every row's first forward pass from its row of first[rows][ld_first],
 *     on hid0's hidden values, or with a NULL hid0 on the row's own.  Nothing is emitted and no draw is read.
 *   between two passes (first NULL, next NULL): emit -- dream_tanh of every output the pass just left in the row's out row
 *     into emit[row][output_size], the frame's place in the segment's buffer -- and feed: dream_next of the same values,
 *     with `noise` and, unless noise == 0, the frame's draws gz[output_size][rows] (ramd_launch_dream_draw's), as the
 *     dense row of the next pass's input row, the soft clip included, on the row's own hidden values.
 *   a call's last (next != NULL): the emit half, and the row dream_next gives into next[row][input_size] instead of the
 *     input row.
 * A workgroup reads its own row's out and hidden rows and draws and no other row's; every word has one writer: no
 * atomics.  gz may be NULL where noise == 0.  All pointers are device pointers. */
typedef struct RamdDreamStep {
  const float *first; /* [rows][ld_first] the rows' first inputs, or NULL                   */
  float *emit;        /* [rows][output_size] the frame to emit (first == NULL)              */
  float *next;        /* [rows][input_size] the rows behind the last frame, or NULL         */
  const float *gz;    /* [output_size][rows] the frame's draws, value-major                 */
  const float *hid0;  /* the hidden row of the first feed, or NULL                          */
  int ld_first;
  int row0, rows;
  float noise;
} RamdDreamStep;
void ramd_launch_dream_step(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b, const RamdDreamStep *p);
/* one frame's draws for it: n values of cheap_gaussian_noise per row, in index order, from the call's generators
 * rng[rows] (rand_ctx; stored back) into gz[n][rows], value-major -- one lane per row, meant for a stream beside the forward pass */
void ramd_launch_dream_draw(ramd_stream_t st, void *rng, float *gz, int rows, int n);

/* rnn_amd_continue_texts and rnn_amd_sample_texts (sample_api.c): launch t = 0 .. of a wave of prompts, ordered by prompt
 * length + max_len; the launch is for the wave's first `rows` rows.  What it does for a row is continue_rule.h's
 * continue_step(plen[row], max_len, t) --
 *   the input row of the next pass from prompt symbol t (the row's prompt starts at prompt[off[row]]; on hid0 at t == 0
 *   unless that is NULL), no draw, no generator, or
 *   the draw of text index t - plen[row] of a row that is not done, from head `head` of alen outputs of its output row
 *   (sample_rule.h: the biased clamped softmax and a draw with the row's own generator rng[row] -- the call's, not
 *   b->rng --, or the best output when bias >= SAMPLE_GREEDY_BIAS) into text[row][max_len], counted in len[row], with
 *   done[row] set (1: it was stop_point, 2: the draw met the attempt cap) -- the row's text and length are fixed from then
 *   on -- and, unless the index was the last, the stop symbol or a failure, the input row of the next pass from the
 *   one-hot of the pick, or
 *   nothing.
 * first != NULL is the sampler's form: every row's prompt is the one symbol first[row] (an int: it may lie above 255),
 * and prompt, off and plen are not read. */
typedef struct RamdTextsContinue {
  const unsigned char *prompt;   /* the wave's prompts behind one another             */
  const unsigned long long *off; /* [rows] where row j's prompt starts                */
  const int *plen;               /* [rows] its length, at least 1                     */
  const int *first;              /* [rows] the rows' one-symbol prompts, or NULL      */
  void *rng;                     /* [rows] rand_ctx: the rows' generators             */
  unsigned char *text;           /* [rows][max_len] the symbols drawn                 */
  int *len;                      /* [rows] how many                                   */
  int *done;                     /* [rows] 0 running, 1 stopped, 2 failed             */
  const float *hid0;
  int row0;
  int alen, head, max_len, t, stop_point;
  float bias;
  int rows;                      /* the launch's rows (the launcher's: a workgroup each) */
} RamdTextsContinue;
void ramd_launch_texts_continue(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b, const RamdTextsContinue *p);
/* a dense loss behind a finished pass, kind RAMD_TOP_SIGMOID_MSE or RAMD_TOP_TANH_SLOPE as above: the rule's answer in
 * place on the first n outputs, its error into o_error; targets is a device array [nrows][ld].  Parrot's always adds the
 * row's sum of (target - a)^2 and one count to the statistics; rnnca's only with stats (rnn_amd_set_automaton_steps alone:
 * the same answers and errors from the row kernel instead of the public call's thread per output) */
void ramd_launch_dense_loss(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b, int row0, int nrows, int kind, int n,
                            const float *targets, int ld, int stats);
/* fast_sigmoid_array in place on the first n outputs of state rows r0 .. r0 + nrows */
void ramd_launch_sigmoid_outputs(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b, int r0,
                                 int nrows, int n);
/* The next ramd_launch_calc_deltas calls may run the weight-delta GEMM in two row halves and call `hook`
 * (ctx, half 0 / 1, first float from ih_delta, floats) after each half's deltas are complete; NULL: off. */
void ramd_set_delta_half_hook(void (*hook)(void *ctx, int half, size_t first_float, size_t n_floats), void *ctx);
/* whether the last ramd_launch_calc_deltas also rebuilt the h_error / i_error images (reads and clears) */
int ramd_calc_wrote_images(void);
/* up to 12 word-wise copies (nwords[g] 32-bit words from src[g] to dst[g]) in one launch */
/* the noise of a coming forward pass of rows [row0, row0 + nrows) into out_noise and the generator states after it
 * into out_states (one of noise_ahead.c's slots), from the generators' current states or -- src_states != NULL -- from
 * those, a loss's draws on: one per head of n_classes but the row's own loss_classes[row], or `skip` draws; the
 * generators themselves are not touched */
void ramd_launch_noise_speculate(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b, int row0, int nrows,
                                 float noise, float *out_noise, void *out_states, const void *src_states,
                                 const int *loss_classes, int n_classes, int skip);
void ramd_launch_segcopy(ramd_stream_t st, int nseg, void *const *dst, const void *const *src,
                         const unsigned *nwords);
/* rebuilds err_a / err_b (bptt->h_error, i_error) from ehi after a calc_deltas */
void ramd_launch_err_writeback(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b,
                               int row0, int nrows);
void ramd_launch_clear_deltas(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b);

/* ---- optimiser (recur-nn.c:454-678): one array at a time ---- */
void ramd_launch_apply(ramd_stream_t st, int method, float *w, const float *delta, float *m,
                       float *aux, size_t n, float rate, float momentum,
                       float momentum_weight, const float *rate_scale_dev);
/* the same for up to three arrays in one launch (top, recurrent, bottom).  gate (or NULL): a device word; where it is 0
 * the launch still sums and stores what `pend` holds as planes, and then leaves weights, momentum and aux arrays alone
 * (rnn_amd_set_classify_steps: the reference's `if (err_sum)`, decided by the loss kernel that ran before) */
void ramd_launch_apply_multi(ramd_stream_t st, int method, int nseg, float *const *w,
                             const float *const *delta, float *const *m, float *const *aux,
                             const size_t *n, const float *rate, float momentum,
                             float momentum_weight, const float *rate_scale_dev,
                             const RamdPendingDelta *pend, const unsigned *gate);
/* the exchange step as kernel-issued peer traffic (kernels_apply.hip: k_apply_xchg, k_xchg_barrier) */
/* sum of word_i * (2 i + 1) mod 2^64 over the arrays in a row, on the device (kernels_apply.hip: k_replica_checksum) */
void ramd_launch_replica_checksum(ramd_stream_t st, int n_arrays, const float *const *arrays, const size_t *n_floats,
                                  unsigned long long *out_dev);
void ramd_launch_xchg_barrier(ramd_stream_t st, unsigned *flags_dev, int rank, int world, unsigned seq,
                              unsigned *abort_word_dev);
void ramd_launch_apply_xchg(ramd_stream_t st, int method, int rank, int world, float *const *w,
                            const float *const *delta, float *const *m, float *const *aux, float *const *delta_out,
                            const size_t *n, const float *rate, float momentum, float mw);
/* conditioning pieces (recur-nn.c:782-855) */
void ramd_launch_scale(ramd_stream_t st, float *a, size_t n, float scale);
void ramd_launch_zero_small(ramd_stream_t st, float *a, size_t n);
void ramd_launch_clamp(ramd_stream_t st, float *a, size_t n, float lo, float hi);
void ramd_launch_tall_poppy(ramd_stream_t st, float *a, size_t n, float threshold,
                            float scale, void *scratch);
void ramd_launch_add_at(ramd_stream_t st, float *a, size_t index, float v);
/* the immediate top-layer update of rnn_bptt_calculate (recur-nn.c:941-964) */
void ramd_launch_fused_updates(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b, int row, float rate,
                               float momentum, float mw, int apply_ih, const float *rs);
/* non-zero once the one-launch BPTT chain has given up (its workgroups were not all
 * resident, or a poll timed out): the results of that launch are not valid */
unsigned ramd_chain_abort_word(void);
unsigned *ramd_abort_word_dev(void);
long ramd_fwd_top_launches(void); /* kernels_forward.hip: launches of the forward + top kernel so far */
long ramd_chain_early_launches(void); /* kernels_chain.hip: launches of k_chain_persist_early so far */
/* the library has created a second stream with work that may run beside the BPTT chain: the chain then stops
 * deriving its workgroups' XCDs from their numbers (kernels_chain.hip) */
void ramd_note_side_stream(void);

/* ---- timing hooks ---- */
void ramd_timing_enable(int enable);
double ramd_timing_ms(int which, long *launches, int reset);
#define RAMD_T_XCHG 5 /* rnn_amd_kernel_time_ms(5, ..): the exchange step between ranks, per generation */
int ramd_timing_begin(ramd_stream_t st, int cls); /* HIP events on st around what follows, when timing is on (else -1) */
void ramd_timing_end(ramd_stream_t st, int i);

#ifdef __cplusplus
}
#endif
#endif
