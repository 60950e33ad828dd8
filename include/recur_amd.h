/* recur_amd.h -- C ABI of librecur_amd.so, the MI355X (gfx950) implementation of
 * Recur's RNN core.
 *
 * Part 1 of this header is the drop-in contract: the public structs, enums and
 * extern functions that the reference exposes in recur-nn.h (the reference has
 * no FFI layer; callers link recur-nn.o / recur-nn-init.o / recur-nn-io.o
 * statically and poke struct fields).  Every
 * declaration cites the reference line it replaces.  Field order, field types
 * and enum values are ABI and therefore identical; everything else in this
 * repository is written from scratch.
 *
 * Part 2 is additive: batched ("training set at once") entry points and the
 * host/device coherence calls a GPU-resident core needs.  A batched call is
 * defined to be equal to looping the per-net call of Part 1 over the set.
 *
 * Plain pointers and sizes only; no C++ or torch types.
 */
#ifndef RECUR_AMD_H
#define RECUR_AMD_H 1

#include <stdint.h>
#include <stddef.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* Short integer names used throughout the reference (recur-common.h:83-91). */
#ifndef RECUR_AMD_NO_SHORT_TYPES
typedef uint64_t u64;
typedef int64_t s64;
typedef uint32_t u32;
typedef int32_t s32;
typedef uint16_t u16;
typedef int16_t s16;
typedef uint8_t u8;
typedef int8_t s8;
typedef unsigned int uint;
#endif

/* Jenkins small-fast 64 bit PRNG state (recur-rng.h:15-20).  It is saved in
 * net files as 32 raw bytes, so the layout is part of the file format. */
typedef struct _rand_ctx {
  uint64_t a;
  uint64_t b;
  uint64_t c;
  uint64_t d;
} rand_ctx;

#define RECUR_RNG_RANDOM_SEED (-1ULL) /* recur-rng.h:13: seed from the clock   */
#define RECUR_RNG_SUBSEED (-2ULL)     /* recur-nn.h:15: seed from parent's rng */

/* Numeric constants of the algorithm (recur-nn.h:19-57, 107). */
#define RANDOM_DAMAGE_FACTOR 0.5f
#define MAX_TOP_ERROR_FACTOR 2.0f
#define MAX_ERROR_GAIN 2.0f
#define ERROR_GAIN_CEILING 1.0f
#define BASE_MIN_ERROR_FACTOR 1e-12f
#define MAX_MIN_ERROR_FACTOR 1e-2f
#define ABS_MIN_ERROR_FACTOR 1e-20f
#define MIN_ERROR_GAIN 1e-8f
#define RNN_HIDDEN_PENALTY 0.0f
#define HIDDEN_MEAN_SOFT_TOP 16.0f
#define INPUT_MEAN_SOFT_TOP 16.0f
#define RNN_INITIAL_WEIGHT_VARIANCE_FACTOR 2.0f
#define WEIGHT_SCALE (1.0f - 1e-6f)
#define RNN_CONDITIONING_INTERVAL 8
#define RNN_TALL_POPPY_THRESHOLD 1.0f
#define RNN_TALL_POPPY_SCALE 0.99f
#define RNN_LAWN_MOWER_THRESHOLD 10.0f
#define RNN_MOMENTUM_WEIGHT 0.5f
#define RNN_COND_USE_OFFSET 16

/* Position of each conditioning task in the 8-generation cycle
 * (recur-nn.h:70-76). */
enum {
  RNN_COND_BIT_SCALE = 0U,
  RNN_COND_BIT_ZERO = 2U,
  RNN_COND_BIT_LAWN_MOWER = 3U,
  RNN_COND_BIT_TALL_POPPY = 4U,
  RNN_COND_BIT_RAND = 6U
};

/* net->flags bits (recur-nn.h:78-103). */
enum {
  RNN_NET_FLAG_OWN_BPTT = 1,
  RNN_NET_FLAG_OWN_WEIGHTS = 2,
  RNN_NET_FLAG_LOG_APPEND = 8,
  RNN_NET_FLAG_LOG_HIDDEN_SUM = 16,
  RNN_NET_FLAG_LOG_WEIGHT_SUM = 32,
  RNN_NET_FLAG_BPTT_ADAPTIVE_MIN_ERROR = 64,
  RNN_NET_FLAG_NO_MOMENTUMS = 128,
  RNN_NET_FLAG_NO_DELTAS = 256,
  RNN_NET_FLAG_BOTTOM_LAYER = 1024,
  RNN_NET_FLAG_AUX_ARRAYS = 2048,

  RNN_COND_USE_SCALE = (1 << (RNN_COND_BIT_SCALE + RNN_COND_USE_OFFSET)),
  RNN_COND_USE_ZERO = (1 << (RNN_COND_BIT_ZERO + RNN_COND_USE_OFFSET)),
  RNN_COND_USE_LAWN_MOWER = (1 << (RNN_COND_BIT_LAWN_MOWER + RNN_COND_USE_OFFSET)),
  RNN_COND_USE_TALL_POPPY = (1 << (RNN_COND_BIT_TALL_POPPY + RNN_COND_USE_OFFSET)),
  RNN_COND_USE_RAND = (1 << (RNN_COND_BIT_RAND + RNN_COND_USE_OFFSET)),

  RNN_NET_FLAG_STANDARD = (RNN_NET_FLAG_OWN_BPTT | RNN_NET_FLAG_OWN_WEIGHTS |
                           RNN_COND_USE_ZERO | RNN_NET_FLAG_LOG_HIDDEN_SUM)
};

/* recur-nn.h:109-119 */
typedef enum {
  RNN_MOMENTUM_WEIGHTED = 0,
  RNN_MOMENTUM_NESTEROV,
  RNN_MOMENTUM_SIMPLIFIED_NESTEROV,
  RNN_MOMENTUM_CLASSICAL,
  RNN_ADAGRAD,
  RNN_ADADELTA,
  RNN_RPROP,
  RNN_LAST_LEARNING_METHOD
} rnn_learning_method;

/* recur-nn.h:121-128 */
typedef enum {
  RNN_INIT_ZERO = 0,
  RNN_INIT_FLAT,
  RNN_INIT_FAN_IN,
  RNN_INIT_RUNS,
  RNN_INIT_LAST
} rnn_init_method;

/* recur-nn.h:130-140 (values are stored in net files) */
typedef enum {
  RNN_RELU = 1,
  RNN_RESQRT,
  RNN_RESERVED_ACTIVATION_1,
  RNN_RESERVED_ACTIVATION_2,
  RNN_RECLIP20 = 5,
  RNN_ACTIVATION_LAST
} rnn_activation;

/* recur-nn.h:142-151 */
typedef enum {
  RNN_INIT_DIST_UNIFORM = 1,
  RNN_INIT_DIST_GAUSSIAN,
  RNN_INIT_DIST_LOG_NORMAL,
  RNN_INIT_DIST_SEMICIRCLE,
  RNN_INIT_DIST_DEFAULT
} rnn_init_distribution;

typedef struct _RecurNN RecurNN;
typedef struct _RecurNNBPTT RecurNNBPTT;
typedef struct _RecurExtraLayer RecurExtraLayer;
typedef struct _RecurErrorRange RecurErrorRange;

/* One net == one stream of the synchronic mini-batch (recur-nn.h:158-186).
 * All pointers are host pointers; see rnn_amd_sync_host() below for when the
 * large arrays they point at are current. */
struct _RecurNN {
  int i_size; /* padded: 1 bias + hidden feedback + real inputs, rounded up to 4 */
  int h_size; /* padded: 1 bias + hidden_size */
  int o_size; /* padded output_size */
  int input_size;
  int hidden_size;
  int output_size;
  int ih_size; /* i_size * h_size */
  int ho_size; /* h_size * o_size */
  uint32_t flags;
  FILE *log;
  float *mem; /* private */
  float *input_layer;
  float *hidden_layer;
  float *output_layer;
  float *ih_weights; /* row major [i_size][h_size] */
  float *ho_weights; /* row major [h_size][o_size] */
  float *real_inputs;
  rand_ctx rng;
  RecurNNBPTT *bptt;
  RecurExtraLayer *bottom_layer;
  char *metadata;
  uint32_t generation;
  float presynaptic_noise;
  rnn_activation activation;
};

/* Training state of one stream (recur-nn.h:188-209). */
struct _RecurNNBPTT {
  int depth;
  int index;
  float *i_error;
  float *h_error;
  float *o_error;
  float *ih_momentum;
  float *ho_momentum;
  float *history; /* ring of depth slots, i_size floats each */
  float *ih_delta;
  float *ho_delta;
  float *ih_delta_tmp;
  float *ih_aux;
  float *ho_aux;
  float *mem; /* private */
  float learn_rate;
  float ih_scale;
  float ho_scale;
  float momentum;
  float momentum_weight;
  float min_error_factor;
};

/* Optional dense layer below the recurrent one (recur-nn.h:211-227). */
struct _RecurExtraLayer {
  float *mem;
  float *weights;
  float *momentums;
  float *aux;
  float *delta;
  float *inputs;
  float *outputs;
  float *i_error;
  float *o_error;
  float learn_rate_scale;
  int input_size;
  int output_size;
  int i_size;
  int o_size;
  int overlap;
};

/* recur-nn.h:230-258 */
struct RecurInitialisationParameters {
  rnn_init_method method;
  rnn_init_method submethod;
  int bias_uses_submethod;
  int inputs_use_submethod;

  float fan_in_sum;
  float fan_in_step;
  float fan_in_min;
  float fan_in_ratio;

  float flat_variance;
  rnn_init_distribution flat_shape;
  double flat_perforation;

  float run_input_probability;
  float run_input_magnitude;
  float run_gain;
  float run_len_mean;
  float run_len_stddev;
  int run_n;
  int run_loop;
  int run_crossing_paths;
  int run_inputs_miss;
  int run_input_at_start;
};

/* Column range of the output layer that carries error (recur-nn.h:260-265);
 * arrays of these end with an entry whose start is negative. */
struct _RecurErrorRange {
  int start;
  int len;
};

/* ----- construction / destruction (recur-nn.h:269-300) ------------------- */
RecurNN *rnn_new(uint input_size, uint hidden_size, uint output_size, u32 flags,
                 u64 rng_seed, const char *log_file, int depth, float learn_rate,
                 float momentum, float presynaptic_noise, rnn_activation activation);
RecurNN *rnn_clone(RecurNN *parent, u32 flags, u64 rng_seed, const char *log_file);
RecurExtraLayer *rnn_new_extra_layer(int input_size, int output_size, int overlap,
                                     u32 flags);
RecurNN *rnn_new_with_bottom_layer(int n_inputs, int r_input_size, int hidden_size,
                                   int output_size, u32 flags, u64 rng_seed,
                                   const char *log_file, int bptt_depth,
                                   float learn_rate, float momentum,
                                   float presynaptic_noise, rnn_activation activation,
                                   int convolutional_overlap);
void rnn_set_log_file(RecurNN *net, const char *log_file, int append_dont_truncate);
void rnn_delete_net(RecurNN *net);
RecurNN **rnn_new_training_set(RecurNN *prototype, int n_nets);
void rnn_delete_training_set(RecurNN **nets, int n_nets, int leave_prototype);

/* ----- weight initialisation (recur-nn.h:287-296, 324, 333-334) ---------- */
void rnn_randomise_weights_clever(RecurNN *net, struct RecurInitialisationParameters *p);
void rnn_randomise_weights_simple(RecurNN *net, const rnn_init_method method);
void rnn_randomise_weights_auto(RecurNN *net);
void rnn_init_default_weight_parameters(RecurNN *net,
                                        struct RecurInitialisationParameters *q);
void rnn_scale_initial_weights(RecurNN *net, float target_gain);
void rnn_print_net_stats(RecurNN *net);
void rnn_perforate_weights(RecurNN *net, float p);
void rnn_zap_non_diagonals(RecurNN *net, int start, int stop, int n_friends);
void rnn_clear_diagonal_only_section(RecurNN *net, uint len, uint friends);

/* ----- the hot path (recur-nn.h:302, 309-322) ---------------------------- */
float *rnn_opinion(RecurNN *net, const float *inputs, float presynaptic_noise);
void rnn_bptt_clear_deltas(RecurNN *net);
void rnn_bptt_advance(RecurNN *net);
void rnn_bptt_calculate(RecurNN *net, uint batch_size);
void rnn_apply_learning(RecurNN *net, int learning_style, float momentum);
float rnn_calculate_momentum_soft_start(float generation, float momentum,
                                        float momentum_soft_start);
void rnn_bptt_calc_deltas(RecurNN *net, int accumulate_delta,
                          RecurErrorRange *top_error_ranges);
void rnn_condition_net(RecurNN *net);
void rnn_log_net(RecurNN *net);
void rnn_forget_history(RecurNN *net, int bptt_too);

/* ----- cold helpers (recur-nn.h:304, 328-331) ---------------------------- */
void rnn_multi_pgm_dump(RecurNN *net, const char *dumpees, const char *basename);
void rnn_weight_noise(RecurNN *net, float deviation);
void rnn_set_momentum_values(RecurNN *net, float x);
void rnn_set_aux_values(RecurNN *net, float x);

/* ----- CDB net files, format version 10 (recur-nn.h:306-307) ------------- */
RecurNN *rnn_load_net(const char *filename);
int rnn_save_net(RecurNN *net, const char *filename, int backup);

/* recur-nn.h:337-349: one "name value" line per call on net->log. */
static inline void rnn_log_float(RecurNN *net, char *name, float value) {
  if (net->log) {
    fprintf(net->log, "%s %.5g\n", name, value);
  }
}
static inline void rnn_log_int(RecurNN *net, char *name, int value) {
  if (net->log) {
    fprintf(net->log, "%s %d\n", name, value);
  }
}

/* ======================================================================== */
/* Part 2: additive entry points.                                            */

/* Number of usable HIP devices.  With 0 devices the host-only functions
 * (construction, initialisation, file I/O, PRNG) still work; every function
 * that has to compute on the device prints a message and abort()s.  There is
 * no CPU fallback. */
int rnn_amd_device_count(void);
/* Select the HIP device (default: LOCAL_RANK from the environment, else 0)
 * and optionally an externally created hipStream_t for all launches. */
void rnn_amd_use_device(int device, void *hip_stream);
void *rnn_amd_current_stream(void);
const char *rnn_amd_version(void);

/* Which copies to bring up to date (bit set). */
enum {
  RNN_AMD_WEIGHTS = 1,   /* ih_weights, ho_weights, bottom layer weights     */
  RNN_AMD_MOMENTUMS = 2, /* ih/ho_momentum, ih/ho_aux                       */
  RNN_AMD_DELTAS = 4,    /* ih_delta, ho_delta                              */
  RNN_AMD_STREAM = 8,    /* this net's history, layers, error vectors, scalars */
  RNN_AMD_ALL_STREAMS = 16, /* the same for every net sharing its weights   */
  RNN_AMD_EVERYTHING = 31
};
/* The device copy of the large arrays is authoritative once a net has been
 * used on the device.  rnn_amd_sync_host makes the host arrays behind the
 * struct pointers current; rnn_amd_host_written tells the library that the
 * caller modified them through the pointers (e.g. net->ih_weights[k] += x).
 * Library functions do both themselves; the per-net calls of Part 1 also keep
 * the small per-stream vectors (input/hidden/output layer, o_error, h_error,
 * i_error, bptt scalars) current on return. */
void rnn_amd_sync_host(RecurNN *net, int what);
void rnn_amd_host_written(RecurNN *net, int what);

/* A training set opened for batched work: nets[0] is the prototype and the
 * others are its rnn_new_training_set() clones. */
typedef struct RnnAmdSet RnnAmdSet;
RnnAmdSet *rnn_amd_set_open(RecurNN **nets, int n_nets); /* (the array is copied: it need not outlive the call) */
void rnn_amd_set_close(RnnAmdSet *set); /* brings the host structs up to date first */
void rnn_amd_set_drop(RnnAmdSet *set);  /* the same without the copy-back: state stays on the device */
int rnn_amd_set_size(const RnnAmdSet *set);

/* == rnn_bptt_advance() on every net of the set. */
void rnn_amd_set_advance(RnnAmdSet *set);

/* == rnn_opinion(nets[j], inputs + j * ld_inputs, nets[j]->presynaptic_noise)
 * for every j.  inputs (host, n_nets rows) may be NULL when the inputs were
 * set by one of the calls below.  If outputs is not NULL the n_nets x o_size
 * answers are copied there (host), which synchronises. */
void rnn_amd_set_opinion(RnnAmdSet *set, const float *inputs, int ld_inputs,
                         float *outputs);
/* One-hot inputs (charmodel-helpers.h:16-33): hot[j] is the input index of
 * stream j (host array). */
void rnn_amd_set_one_hot_opinion(RnnAmdSet *set, const int *hot, float *outputs);

/* Upload n_nets x o_size error rows (host) into bptt->o_error of the streams. */
void rnn_amd_set_put_o_error(RnnAmdSet *set, const float *o_error, int ld);
/* Device version of net_error_bptt's loss (charmodel-predict.c:18-27):
 * o_error = onehot(target) - softmax(output) with the reference's fast_expf
 * (badmaths.h:14-29, 71-141).  Per stream it adds the error of the target
 * class, log2(1 - that error) (capped, charmodel-helpers.h:11-13) and the
 * "winner == target" count into device accumulators read by
 * rnn_amd_set_read_stats.
 *
 * ROWS THAT ARE NOT FINITE.  This holds for every loss of this part (the softmax, class-group, multi-head and sigmoid
 * errors, the text steps, rnn_char_cross_entropy and rnn_char_multi_cross_entropy) and for the batched calls below
 * (rnn_amd_run_texts and _heads, rnn_amd_trace_texts, rnn_amd_classify_texts, rnn_amd_run_sequences, their _from forms).
 * The reference's fast_expf halves its argument's exponent in a loop that an infinity never leaves; the library's
 * (csrc/fast_exp_rule.h) is the same function on every finite float and gives NaN for an argument that is not finite.
 * An unbounded activation or a diverged net can overflow an output row, and rnn_amd_run_sequences takes the caller's
 * floats, so:
 *   - A softmax -- a head, a class group, a whole output row -- that contains an infinity or a NaN has no likelihoods.
 *     Every float the call derives from it is NaN: its errors, likelihoods and log-likelihoods, and the per-text and
 *     per-set sums they are added into (error, entropy, the cross entropies, sums and sums of squares).  The sigmoid of
 *     an output that is not finite is NaN, and so is its error; it is elementwise and touches no other output.
 *   - The integer by-products of such a softmax -- the best guess, a winner byte, `correct` -- are unspecified.  `count`
 *     is not: the step is counted.
 *   - Every other head, group, row, stream or text of the same call is untouched, bit for bit; outputs that take part in
 *     no softmax or sigmoid (the columns of rnn_amd_run_sequences outside every group) are copied as they are.
 *   - Every call returns.
 *   - Parrot's tanh loss (rnn_amd_set_tanh_error and the calls built on it) is the exception to the infinity rule: it
 *     follows fast_tanhf, which clamps.  An infinite output becomes exactly +-1.0f, its slope 1 - a * a exactly 0 and its
 *     error exactly 0 for a finite target; a NaN output gives a NaN answer and a NaN error.  Elementwise as well.
 * A NaN error row then spreads through the deltas into the weights, as it would on any path: the contract is about the
 * call that meets the row.  The samplers (rnn_amd_sample_texts, rnn_amd_continue_texts) say below what they do with an
 * output row without a total: the row ends at the attempt cap and the call returns -1. */
void rnn_amd_set_softmax_error(RnnAmdSet *set, const int *target);

/* == for every j with (active == NULL || active[j]):
 *      rnn_bptt_calc_deltas(nets[j], accumulate || not the first, ranges)
 * i.e. with accumulate == 0 the deltas are zeroed first, exactly as the
 * reference callers do with "j ? 1 : 0" (charmodel-predict.c:309). */
void rnn_amd_set_calc_deltas(RnnAmdSet *set, int accumulate,
                             RecurErrorRange *top_error_ranges, const u8 *active);

/* The loss of gstclassify's train_channel (gstclassify.c:2070-2119) for every stream, on
 * the device, after an rnn_amd_set_opinion: the outputs are n_groups class groups
 * (group i = outputs [group_offset[i], group_offset[i] + group_size[i])); for stream j and
 * group i with 0 <= targets[j * n_groups + i] < group_size[i] the group's error becomes
 * -softmax with +1 on the target, otherwise zeros (the caller passes -1 where the reference
 * skips a group: unknown target, ignored windows, the balanced-sampling draw); if any group
 * of a stream was trained its whole error row is multiplied by error_weight (may be NULL).
 * trained[j] (may be NULL) receives whether stream j has anything to back-propagate: pass
 * it to rnn_amd_set_calc_deltas as the active mask.  Wins, wrongness and trained groups
 * add to the correct / error / count accumulators of rnn_amd_set_read_stats. */
void rnn_amd_set_grouped_softmax_error(RnnAmdSet *set, int n_groups, const int *group_offset,
                                       const int *group_size, const int *targets,
                                       const float *error_weight, u8 *trained);
/* One generation of the multi-head text model (charmodel-multi-predict.c:17-58, 244-256) for
 * every stream of the set: rnn_bptt_advance, a one-hot opinion of hot[j] with the net's
 * presynaptic noise, the multi-head softmax error against next[j] -- the head
 * target_class[j] always, every other head with probability `leakage` drawn from the
 * stream's own generator --, and rnn_bptt_calc_deltas with the error ranges that loss
 * produces.  accumulate applies to the first stream; the others accumulate.  The output
 * layer is output_size / alphabet_len heads (at most 64).  Loss statistics of the own
 * head go to the accumulators rnn_amd_set_read_stats reads (error, entropy, count). */
void rnn_amd_set_multi_step_deltas(RnnAmdSet *set, const int *hot, const int *next,
                                   const int *target_class, int alphabet_len, float leakage,
                                   int accumulate);
/* The same generation with its update, as ONE call: rnn_amd_set_multi_step_deltas(..., accumulate 0) + rnn_apply_learning(
 * nets[0], learning_style, momentum) (charmodel-multi-predict.c:244-262: text_train's step and its rnn_apply_learning).
 * The same results; knowing the update that follows, the weight-delta GEMM carries it out in its own epilogue where the
 * rule is ADAGRAD (the trainer's default) or the momentum rule -- no optimiser launch (round 6). */
void rnn_amd_set_multi_step(RnnAmdSet *set, const int *hot, const int *next, const int *target_class,
                            int alphabet_len, float leakage, int learning_style, float momentum);

/* The two halves of rnn_amd_set_multi_step_deltas with the text on the device (stream j reads
 * text[o], is scored against text[o + 1], o as in rnn_amd_set_char_step): the loss leaves
 * o_error and one error-range list per stream on the device, the deltas call consumes them.
 * In between a caller may apply the previous batch's deltas, as the reference's text_train
 * does (charmodel-multi-predict.c:244-252).  target_class (host, n_nets) may be NULL to keep
 * the classes of the previous call. */
void rnn_amd_set_multi_text_loss(RnnAmdSet *set, int i, const int *target_class, int alphabet_len,
                                 float leakage);
void rnn_amd_set_multi_calc_deltas(RnnAmdSet *set, int accumulate);
/* rnn_bptt_advance (if advance) + one_hot_opinion of each stream's text symbol and nothing
 * else (rnn_char_multitext_spin's step, charmodel-multi-predict.c:293-297); 0 <= i < len */
void rnn_amd_set_text_opinion(RnnAmdSet *set, int i, int advance);
/* rnnca's loss on the device (gstrnnca.c:701-714, train_net) after an rnn_amd_set_opinion:
 * for every stream the first n outputs become their fast_sigmoid IN PLACE (badmaths.h:33-44,
 * as the reference's fast_sigmoid_array(answer, answer, 3) does to output_layer) and
 * o_error[i] = a (1 - a) (targets[j * ld + i] - a); the error never visits the host. */
void rnn_amd_set_sigmoid_mse_error(RnnAmdSet *set, const float *targets, int ld, int n);
/* rnn_amd_set_opinion (outputs not fetched) + rnn_amd_set_sigmoid_mse_error, resp. + rnn_amd_set_grouped_softmax_error,
 * as ONE call: what train_net does per cell between two calc_deltas (gstrnnca.c:693-714) and train_channel per channel
 * (gstclassify.c:2070-2119).  Same results as the two calls; the hidden layer's activation, the output layer, the loss
 * and the top layer's backprop then share one launch (one workgroup per stream: the hidden row, the outputs and the
 * output error never leave the CU), and the rnn_amd_set_calc_deltas that follows -- with `trained` as its active mask
 * in the class-group case, no error ranges -- finds the top layer's backprop done.  Shapes outside that launch's
 * reach (more than 64 outputs, a bottom layer, presynaptic noise) simply make the two calls. */
void rnn_amd_set_opinion_sigmoid_mse(RnnAmdSet *set, const float *inputs, int ld_inputs, const float *targets, int ld,
                                     int n);
void rnn_amd_set_opinion_grouped_softmax(RnnAmdSet *set, const float *inputs, int ld_inputs, int n_groups,
                                         const int *group_offset, const int *group_size, const int *targets,
                                         const float *error_weight, u8 *trained);
/* rnnca's maybe_learn for every trainer at once (gstrnnca.c:693-740) as ONE call, the dense-input counterpart of
 * rnn_amd_set_char_step: rnn_bptt_clear_deltas, the opinion of `inputs`, the sigmoid-slope loss against `targets` (first n
 * outputs), rnn_bptt_calc_deltas for every stream, rnn_apply_learning(net, learning_style, momentum).  The same results
 * as rnn_bptt_clear_deltas + rnn_amd_set_opinion_sigmoid_mse + rnn_amd_set_calc_deltas(set, 1, NULL, NULL) +
 * rnn_apply_learning; knowing the update that follows, the weight-delta GEMM carries it out in its own epilogue where the
 * rule is the momentum rule (no optimiser launch: 14 us of 879 at 2048 / 512 / 10).  The caller advances the ring first
 * (rnn_amd_set_advance) if its trainer has a history, as the synthetic configs[4] driver does. */
void rnn_amd_set_dense_step_sigmoid_mse(RnnAmdSet *set, const float *inputs, int ld_inputs, const float *targets, int ld,
                                        int n, int learning_style, float momentum);
/* ---- parrot's trainer (gstparrot.c: train_net 464-477, maybe_learn 487-554) on the device ----
 * The loss after an rnn_amd_set_opinion: for every stream the first n outputs become their fast_tanhf IN PLACE
 * (badmaths.h:55-68, tanh_opinion) and o_error[i] = (1 - a * a) * (targets[j * ld + i] - a), operation for operation
 * (csrc/parrot_rule.h: the square, the slope, the difference and the product are four fp32 roundings, none fused).
 * Outputs and error columns from n on stay what they were; it works at any output size.  targets: host [n_nets][ld].
 *
 * STATISTICS.  Per stream-step the loss adds the sum over the n outputs of (target - a)^2 to `error` and 1 to `count`
 * of rnn_amd_set_read_stats, so error / (count * n) is the mean squared error and a training loop has a progress figure
 * without fetching anything per generation.  The order of that sum is the library's own (wave reductions, then the waves
 * in order): it is held to a float64 restatement at 1e-4 relative, not bit for bit.
 *
 * OUTPUTS THAT ARE NOT FINITE follow fast_tanhf, and this DIFFERS from the sigmoid's rule above, where an infinity is
 * NaN: an infinite output is clamped to +-1.0f, so its slope and its error are exactly 0 for a finite target; a NaN
 * output gives a NaN answer and a NaN error (and a NaN `error` sum for its stream).  Both are elementwise: no other
 * output, row or stream is touched, and every call returns.
 *
 * THE SUM OVER CHANNELS.  The plugin calls rnn_bptt_calc_deltas(net, 0, NULL) for every channel (gstparrot.c:475), which
 * zeroes the sums each time: of n channels only the last one's deltas reach the update.  These calls SUM over all the
 * streams of the set, as every other trainer here and in the reference does.  A set of ONE net is the plugin with one
 * channel exactly; the overwrite is not emulated. */
void rnn_amd_set_tanh_error(RnnAmdSet *set, const float *targets, int ld, int n);
/* rnn_amd_set_opinion (outputs not fetched) + rnn_amd_set_tanh_error as ONE call.  Same results as the two calls; where
 * the text top launch takes the shape (up to 256 outputs -- parrot's 256 bins --, no bottom layer, no presynaptic noise;
 * RECUR_AMD_DENSE_TOP=0 switches it off) the hidden layer's activation, the output layer, the loss and the top layer's
 * backprop share one launch, every output column a thread of its own, and the rnn_amd_set_calc_deltas that follows finds
 * the top layer's backprop done.  Elsewhere it simply makes the two calls. */
void rnn_amd_set_opinion_tanh_error(RnnAmdSet *set, const float *inputs, int ld_inputs, const float *targets, int ld,
                                    int n);
/* maybe_learn's body for every channel at once, as ONE call: rnn_bptt_clear_deltas, then per stream rnn_bptt_advance
 * (train_net advances; do NOT call rnn_amd_set_advance as well), the opinion of `inputs`, the loss against `targets`,
 * rnn_bptt_calc_deltas SUMMED over the streams (see above), and rnn_apply_learning(nets[0], learning_style, momentum).
 * The same results as rnn_bptt_clear_deltas + rnn_amd_set_advance + rnn_amd_set_opinion_tanh_error +
 * rnn_amd_set_calc_deltas(set, 1, NULL, NULL) + rnn_apply_learning; knowing the update that follows, the weight-delta GEMM
 * carries it out in its own epilogue where the rule is the momentum rule.  rnn_condition_net is the caller's. */
void rnn_amd_set_dense_step_tanh(RnnAmdSet *set, const float *inputs, int ld_inputs, const float *targets, int ld, int n,
                                 int learning_style, float momentum);
/* n_steps such generations from ONE block of frames: parrot's target at generation t is its input at generation t + 1.
 * frames: host [n_steps + 1][n_nets][ld], ld >= max(input_size, n).  The block goes up once, into a buffer of the
 * engine's that grows on demand and is freed with the engine; generation t is rnn_amd_set_dense_step_tanh's work with
 * inputs frames[t] and targets frames[t + 1], read where they lie on the device, followed by rnn_condition_net(nets[0])
 * when `condition` is not 0 (gstparrot.c:544-545).  There is no upload per generation and no synchronisation between the
 * generations (the block's own upload is waited for where it is larger than the 1 MB mailbox; the conditioning's random
 * damage, where the net's flags ask for it, draws on the host).  The last frame of a block is the first of the next: a
 * caller chains blocks.  n_steps < 1, NULL frames, n outside the outputs or a too-small ld abort with a message (which
 * blocks it takes is stated once, csrc/parrot_rule.h: parrot_block_refusal, and tested there without a device).  (A set with a bottom layer
 * takes its rows from the host, generation by generation.) */
void rnn_amd_set_dense_steps_tanh(RnnAmdSet *set, const float *frames, int ld, int n_steps, int n, int learning_style,
                                  float momentum, int condition);
/* fill_frame's step after the opinion (gstrnnca.c:813-814): fast_sigmoid in place on the first
 * n outputs of every net of the set (training or forward-only clones); outputs (host, n_nets x
 * o_size, may be NULL) receives the answer rows, which synchronises. */
void rnn_amd_set_sigmoid_outputs(RnnAmdSet *set, int n, float *outputs);

/* Text on the device, for a host-free epoch loop (charmodel-predict.c:288-311).  The resident text belongs
 * to the set's ENGINE (the weight-owning net and its clones): every set opened on the same nets sees the
 * text loaded last, and a text step at a position outside it aborts with a message. */
void rnn_amd_set_load_text(RnnAmdSet *set, const u8 *text, int len);
/* One generation of rnn_char_epoch's multi-tap branch for text position i:
 * stream j reads text[off] and is scored against text[off + 1], with
 * off = i + j * ((len - 1) / n_nets), wrapped at len - 1;
 * advance, one-hot opinion, softmax error, calc_deltas(j ? 1 : 0), and then
 * rnn_apply_learning(nets[0], learning_style, momentum).  Nothing is copied to
 * the host. */
void rnn_amd_set_char_step(RnnAmdSet *set, int i, int learning_style, float momentum);
/* The same for ONE net on the fused single-net path (charmodel-predict.c:312-321): advance, opinion of
 * text[i], the loss against text[i + 1] on the device, rnn_bptt_calculate(net, batch_size); the caller
 * sets bptt->momentum first, as the reference's loop does.  No host round trip per symbol. */
void rnn_amd_set_char_step_fused(RnnAmdSet *set, int i, unsigned batch_size);

typedef struct RnnAmdStats {
  double error;   /* sum of target-class errors                */
  double entropy; /* sum of capped log2(1 - error)            */
  long correct;   /* count of winner == target                */
  long count;     /* stream-timesteps accumulated              */
  double bptt_depth_sum; /* sum of executed BPTT steps          */
  double hidden_zeros;   /* sum over stream-steps of the zero fraction of hiddens */
} RnnAmdStats;
/* Reads (and optionally clears) the device accumulators; synchronises. */
void rnn_amd_set_read_stats(RnnAmdSet *set, RnnAmdStats *stats, int clear);

/* FOR TESTS AND TOOLS: what the engine behind the set has put off until a later call needs it, as bits.  The library
 * settles all of it by itself, whichever call comes next; no caller has to ask.  The query exists so that a test of one
 * settlement route can tell that the state it means to settle was there.  It launches nothing, copies nothing and
 * changes nothing.
 *   RNN_AMD_DEFERRED_IH_PLANES  the last rnn_amd_set_calc_deltas (accumulate 0) left ih_delta as unsummed split-K planes
 *   RNN_AMD_DEFERRED_HO_PLANES  ... and ho_delta
 *   RNN_AMD_DEFERRED_CLEAR      an rnn_bptt_clear_deltas has not been carried out yet
 *   RNN_AMD_DEFERRED_IMAGES     the h_error / i_error images of the last delta call's rows have not been rebuilt yet
 *   RNN_AMD_DEFERRED_TOP_DONE   the top layer's backprop of exactly this set's rows has been done with their loss */
#define RNN_AMD_DEFERRED_IH_PLANES 1
#define RNN_AMD_DEFERRED_HO_PLANES 2
#define RNN_AMD_DEFERRED_CLEAR 4
#define RNN_AMD_DEFERRED_IMAGES 8
#define RNN_AMD_DEFERRED_TOP_DONE 16
int rnn_amd_set_deferred(const RnnAmdSet *set);

/* ---- multi-GPU: one process per GPU, streams sharded, one all-reduce per generation ----
 * The reference sums the deltas of all streams in one process (recur-nn.c:724-739 over the
 * sharing of recur-nn-init.c:232-241); these calls distribute that sum.  rank 0 obtains an
 * id (128 bytes) and hands it to every rank by whatever means the launcher has (a file, a
 * pipe, MPI, torchrun's store); every rank then joins with the device it selected with
 * rnn_amd_use_device.  While a group is joined, rnn_amd_set_char_step (and
 * rnn_amd_set_dist_all_reduce_deltas for callers that drive calc_deltas / apply_learning
 * themselves) sum ih_delta||ho_delta over the ranks with ONE RCCL all-reduce on the
 * library's stream between the deltas and the update; rnn_amd_set_open shards the text
 * offsets as rnn_amd_set_shard(rank * n_nets, world * n_nets) unless told otherwise.
 * COLLECTIVE BEHAVIOUR of host draws: on a net whose training set is sharded over the group
 * (made by rnn_amd_new_training_set_shard with n_local != global_count, opened with rnn_amd_set_open
 * as ALL of its engine's training streams while the group is joined -- until that set is closed or
 * dropped --, or given a shard by rnn_amd_set_shard), rnn_weight_noise,
 * rnn_perforate_weights and the random damage of rnn_condition_net draw from RANK 0's generator
 * (a 32-byte broadcast) so that the replicas stay identical: EVERY rank must make that call on
 * its replica.  Nets that are not part of a sharded set (validation / confabulation clone
 * families of their own, side nets) are untouched by the group and draw locally.
 * All return 0 on success, -1 on failure (RCCL not loadable, bad arguments), with two exceptions in
 * rnn_amd_dist_init, which END THE PROCESS with _exit(86) after a message on stderr: a rank that has waited
 * RECUR_AMD_RCCL_INIT_TIMEOUT seconds (default 180) for the others inside ncclCommInitRank -- the helper thread
 * sitting in RCCL cannot be cancelled, and a process that has touched the GPU must not re-exec or retry --, and a
 * communicator whose rank / size are not the ones asked for.  A launcher sees exit status 86 of that rank. */
#define RNN_AMD_DIST_ID_BYTES 128
int rnn_amd_dist_get_id(void *id);
int rnn_amd_dist_init(int rank, int world, const void *id);
void rnn_amd_dist_finalize(void);
int rnn_amd_dist_rank(void);  /* 0 when no group is joined */
int rnn_amd_dist_world(void); /* 1 when no group is joined */
/* ---- the exchange step WITHOUT a collective library: reduce-scatter -> sharded optimiser -> all-gather as
 * kernel-issued peer traffic (SURVEY.md section 8e's alternative; the sum it distributes is recur-nn.c:734-739,
 * the update it shards recur-nn.c:601-678).  Every rank owns 1 / world of each weight array; ONE kernel per
 * generation adds the ranks' local delta sums for its range in rank order through peer pointers (replicas stay
 * bit-identical), updates its own weights and momentum there -- the optimiser state of a range lives on its owner
 * only -- and stores the new weights into every rank's weight array; two arrival barriers (kernels on the
 * library's stream that count in host memory all ranks have mapped) keep the ranks' generations apart.  No RCCL
 * launch, no separate all-reduce pass.  Up to 8 ranks, no bottom layer, ranks on GPUs with peer access (or on one
 * GPU: the tests' emulation).  OPT-IN: the RCCL all-reduce above stays the default until a multi-GPU node has
 * measured both.
 *   1. each rank: rnn_amd_set_exchange_export(set, blob)  -- 256 bytes naming its delta and weight arrays (IPC
 *      handles; same-process peers are recognised and take the plain pointers);
 *   2. the launcher hands every blob to every rank (a file, shared memory, a pipe) and provides `counters`: 64 bytes
 *      of zeroed host memory that ALL ranks have mapped (MAP_SHARED memory made before fork, or a file in /dev/shm);
 *      they need no zeroing between sessions (round 6): the barriers count on from where words 0 .. 7 stand at the
 *      join, words 8 .. 15 carry the join's own rendezvous, named by a token made of the session's blobs;
 *   3. each rank: rnn_amd_set_exchange_join(set, rank, world, blobs, counters, 0) -- COLLECTIVE: it returns when every
 *      rank of the session has called it (RECUR_AMD_XCHG_JOIN_TIMEOUT seconds at most, default 120: -1 then); from then
 *      on rnn_amd_set_char_step runs deltas -> barrier -> sharded update -> barrier.
 * lockstep != 0: the ranks are sets of ONE process driven by one thread (counters may be NULL): no barriers are
 * launched, the caller gives the order -- rnn_amd_set_char_step_deltas on every rank, then
 * rnn_amd_set_apply_exchange on every rank.  After a step ih_delta || ho_delta hold the sum over the ranks in the
 * rank's OWN range only, and momentum / aux arrays are current in the own range only (rnn_amd_set_exchange_range).
 * With ONE rank rnn_amd_set_char_step is the plain generation (nothing to exchange); the arrays reached through peer
 * pointers are ordinary device allocations whose visibility between ranks rests on kernel boundaries: on GPUs of
 * different devices that has not run yet.
 * Returns 0, or -1 with a message (a peer's arrays cannot be opened, bad arguments). */
#define RNN_AMD_EXCHANGE_BLOB_BYTES 256
/* A 64-bit checksum of this rank's replica: sum over the 32-bit words of ih_weights || ho_weights (with_momentum: ||
 * ih_momentum || ho_momentum) of word_i * (2 i + 1) mod 2^64.  through_kernel != 0: formed by a kernel on the library's
 * stream, i.e. through the caches the path's own kernels read the arrays through; 0: over a device-to-host copy.  The
 * replicas of a sharded run are bit-identical (RCCL: every rank adds the same sum; kernel-issued: every range has one
 * owner), so a launcher compares the ranks' values after a run -- and the two readings of ONE rank, which differ only
 * if a peer's stores did not reach what this rank's kernels see (bench.py does both and exits non-zero).  In the
 * kernel-issued exchange momentum lives in the owner's range only: compare weights there.  Synchronises. */
uint64_t rnn_amd_set_replica_checksum(RnnAmdSet *set, int with_momentum, int through_kernel);
void rnn_amd_set_exchange_export(RnnAmdSet *set, void *blob);
int rnn_amd_set_exchange_join(RnnAmdSet *set, int rank, int world, const void *blobs, void *counters, int lockstep);
void rnn_amd_set_exchange_leave(RnnAmdSet *set);
/* the update of rnn_apply_learning through the exchange (the second half of rnn_amd_set_char_step) */
void rnn_amd_set_apply_exchange(RnnAmdSet *set, int learning_style, float momentum);
/* this rank's range of the recurrent (which = 0) or top-layer (1) arrays, in floats */
void rnn_amd_set_exchange_range(const RnnAmdSet *set, int which, size_t *first, size_t *count);

/* in-place sum over the ranks of a device buffer of floats, on the library's stream */
void rnn_amd_dist_all_reduce(void *device_buffer, size_t n_floats);
/* max over the ranks of a host value / a barrier (the timing bracket of a benchmark) */
double rnn_amd_dist_max(double x);
void rnn_amd_dist_barrier(void);
/* rnn_new_training_set (recur-nn-init.c:221-243) for one shard of a set of global_count
 * streams: the prototype's generator hands out the clone seeds of ALL global streams in
 * order (recur-nn-init.c:300-305), this process keeps streams [global_first, global_first
 * + n_local): nets[0] is the prototype (which, for global_first > 0, takes the generator of
 * global stream global_first), nets[j] the clone of global stream global_first + j.  With
 * global_first 0 and global_count == n_local it is rnn_new_training_set. */
RecurNN **rnn_amd_new_training_set_shard(RecurNN *prototype, int n_local, int global_first,
                                         int global_count);

/* Multi-GPU: when set, ih_delta||ho_delta of the set live in the caller's
 * device buffer (ih_size + ho_size floats, ih first), so that the caller can
 * all-reduce it (RCCL) between calc_deltas and apply_learning.  Pass NULL to
 * go back to library-owned storage. */
void rnn_amd_set_external_delta(RnnAmdSet *set, void *device_buffer);
/* When the streams of one logical training set are sharded over several
 * processes (one per GPU), this set holds global streams
 * [global_first, global_first + n_nets) of global_count: rnn_amd_set_char_step
 * then spaces the text offsets over global_count streams
 * (charmodel-predict.c:273, 295).  Default: global_first 0, global_count n_nets. */
void rnn_amd_set_shard(RnnAmdSet *set, int global_first, int global_count);
/* Split rnn_amd_set_char_step for that use: everything up to and including
 * calc_deltas, then the update. */
void rnn_amd_set_char_step_deltas(RnnAmdSet *set, int i);
/* sums the set's ih_delta||ho_delta over the joined ranks (no-op without a group) */
void rnn_amd_set_dist_all_reduce_deltas(RnnAmdSet *set);
/* One net run over an encoded text without leaving the device: a one-hot opinion
 * (charmodel-helpers.h:16-33) of text[i] for every i < len - 1, and from i = skip on
 * the log2 of the softmax probability of text[i + 1] (capped at -100 like
 * capped_log2f).  Returns the sum of the logs: get_cross_entropy's loop
 * (charmodel-predict.c:62-76) without its final division; with skip >= len - 1 it is
 * rnn_char_prime's loop (407-416).  Works for nets with or without bptt. */
double rnn_amd_run_text(RecurNN *net, const u8 *text, int len, int skip);
/* The same for a net whose output row is output_size / alphabet_len heads: sums[c] (room for
 * that many doubles) receives head c's sum of capped log2 softmax(head c)[text[i + 1]] over
 * i in [skip, len - 1): rnn_char_multi_cross_entropy's loops (charmodel-multi-predict.c:388-403)
 * without the final negation and division. */
void rnn_amd_run_text_heads(RecurNN *net, const u8 *text, int len, int skip, int alphabet_len,
                            double *sums);
/* Many texts against one net in ONE batched device run: the set form of rnn_amd_run_text.  For every k, sums[k] is what
 * rnn_amd_run_text(c_k, texts[k], lens[k], skips[k]) returns, where c_k is a forward-only clone of `net` whose hidden
 * row starts as a copy of net's hidden row at the moment of the call -- with one-hot inputs and no bottom layer the
 * hidden row is the only state that carries from symbol to symbol (charmodel-helpers.h:16-33).  The texts do not see
 * one another (the reference's text-cross-entropy.c:156-200 carries the net's state from one file into the next, so its
 * figures depend on the order of its arguments; these do not), noise is 0 and no generator is touched
 * (charmodel-predict.c:62-76), and `net` itself -- host and device copies, generator included -- is left exactly as it
 * was.  The clones are state rows of the engine's own, not nets; the texts run side by side, longest first, in waves of
 * up to 256 rows with one device synchronisation per wave.
 * skips may be NULL (all zeros); a text with len < 2 scores 0.0; n_texts == 0 returns 0 and touches nothing.
 * A text whose output row holds an infinity or a NaN at a scored step has a NaN sum; every other text is untouched and the
 * call returns ("Rows that are not finite" at rnn_amd_set_softmax_error above -- it covers every batched call here).
 * Returns 0, or -1 with a message on stderr and nothing computed (checked before anything needs a device): n_texts < 0,
 * a NULL array with n_texts > 0, heads that do not divide the output row, a net with a bottom layer -- the layer has
 * ONE input buffer shared by every clone (recur-nn-init.c:345-346, charmodel-helpers.h:20-31), which leaves
 * "independent clones" of such a net undefined. */
int rnn_amd_run_texts(RecurNN *net, const u8 *const *texts, const int *lens, const int *skips, int n_texts,
                      double *sums); /* sums[n_texts] */
/* The same for a net whose output row is output_size / alphabet_len heads (rnn_amd_run_text_heads,
 * charmodel-multi-predict.c:388-403): sums[k * n_heads + c] is head c's sum for text k. */
int rnn_amd_run_texts_heads(RecurNN *net, const u8 *const *texts, const int *lens, const int *skips, int n_texts,
                            int alphabet_len, double *sums); /* [n_texts][output_size / alphabet_len] */
/* Many texts TRACED symbol by symbol in one batched device run: rnn_amd_run_texts(_heads) with every float it adds handed
 * back instead of their sum.  With n_heads = alphabet_len ? output_size / alphabet_len : 1 and alen = alphabet_len ?
 * alphabet_len : output_size, for every text k with lens[k] >= 2, every t in [0, lens[k] - 1) and every head c:
 *     logp[k][t * n_heads + c]   the float rnn_amd_run_texts(_heads) adds into its double at step t: capped_log2f
 *         (charmodel-helpers.h:11-13) of softmax(head c)[texts[k][t + 1]] after texts[k][0 .. t] were fed as one-hot
 *         opinions; -100 for a symbol outside the head.  Added one after another in a double from skips[k] on they are
 *         that call's sum, bit for bit.
 *     guess[k][t * n_heads + c]  what softmax_best_guess (badmaths.h:113-141) returns for that head at that step: the
 *         index of the largest likelihood after the division, the lowest index among equal ones.
 * guess may be NULL (no guesses are taken); guess[k] and logp[k] of a text shorter than 2 symbols may be NULL, and nothing
 * is written for such a text, nor behind the (lens[k] - 1) * n_heads entries of any other.  There is no skips: every step
 * is traced and the caller ignores what it wants.
 * Everything else is rnn_amd_run_texts's contract: each text runs on a forward-only clone that starts from net's hidden
 * row at the moment of the call, the texts do not see one another, there is no noise and no generator is touched, `net`
 * -- host and device copies -- is left exactly as it was; the rows go longest first, in waves of up to 256, with one
 * device synchronisation per wave.
 * Memory: a wave's trace stays on the device until the wave's one synchronisation and comes back in one copy -- 5 bytes
 * per traced value (4 without guesses) on the device and as many in a host staging buffer, for the first wave (the 256
 * longest texts) the sum of (lens[k] - 1) * n_heads of them.
 * Returns 0; n_texts == 0, or no text of two symbols, returns 0 at once and asks for no device.  Returns -1 with a message
 * on stderr and nothing computed, before anything needs a device: all that rnn_amd_run_texts_heads refuses, with
 * alphabet_len == 0 allowed here; a NULL logp with n_texts > 0; a NULL logp[k], or with guess a NULL guess[k], for a text
 * of 2 or more symbols; guess with alen > 256, whose indices do not fit a byte. */
int rnn_amd_trace_texts(RecurNN *net, const u8 *const *texts, const int *lens, int n_texts, int alphabet_len,
                        float *const *logp, u8 *const *guess);
/* Many texts DRAWN from one net in one batched device run: the generative counterpart of rnn_amd_run_texts.  Row k of
 * `out` is what this loop writes on a forward-only clone c_k of `net` whose hidden row starts as a copy of net's hidden
 * row at the moment of the call and whose generator is init_rand64(seeds[k]) (recur-rng.h:33-43):
 *     sym = first[k];
 *     repeat up to max_len times: sym = the next symbol after feeding sym; write sym; stop after writing stop_point
 * "the next symbol" being rnn_char_confabulate's (charmodel-predict.c:29-60): one forward pass on the one-hot of sym, the
 * clamped softmax of head `head` of alphabet_len outputs, sharpened by `bias` (badmaths.h:71-156), and a draw from it with
 * c_k's generator; with bias >= 100 the best output (the last of equal maxima) and no draw.  alphabet_len == 0: one head
 * as wide as the output row.  stop_point < 0: no stop symbol.  out_lens[k] counts the symbols written, the stop symbol
 * included; nothing is written behind them.  rng_out[k] (rng_out may be NULL) is c_k's generator afterwards.
 * The draws are made on the device, from probabilities computed there: against a host computation of the same net they
 * can differ where a draw falls within rounding of a boundary between two symbols, and from that symbol on the texts
 * part -- each is a valid sample, and the same call gives the same bytes every time.
 * `net` itself -- host and device copies, hidden row, generator, what it computes next -- is left exactly as it was.  The
 * clones are state rows of the engine's own; the rows run side by side in waves of up to 256 with one device
 * synchronisation per wave, and one more every 64 steps to end a wave whose every row has met its stop symbol.
 * Returns 0; n_texts == 0 or max_len == 0 returns 0 at once (lengths zeroed, no device asked for).  Returns -1 when a row's
 * draw failed (64 attempts without a pick: an output row whose softmax has no total, NaN for one) -- that row ends where
 * it failed, the others are complete.  Returns -1 with a message on stderr and nothing computed, before anything needs a
 * device: a net with a bottom layer (as rnn_amd_run_texts), n_texts < 0 or max_len < 0, a NULL first, seeds, out or
 * out_lens with n_texts > 0, a first[k] outside [0, input_size), heads that do not divide the output row, a head out of
 * range. */
int rnn_amd_sample_texts(RecurNN *net, const int *first, const u64 *seeds, int n_texts, int max_len, float bias,
                         int stop_point, int alphabet_len, int head, u8 *out /* [n_texts][max_len] */, int *out_lens,
                         rand_ctx *rng_out /* [n_texts] or NULL */);
/* Many PROMPTS continued by one net in one batched device run: rnn_amd_sample_texts with a prompt per row in front of
 * the draws.  Row k of `out` is what this loop writes on a forward-only clone c_k of `net` whose hidden row starts as a
 * copy of net's hidden row at the moment of the call and whose generator is init_rand64(seeds[k]):
 *     feed prompts[k][0 .. prompt_lens[k] - 2] as one-hot opinions: nothing is drawn, the generator is not touched
 *         (rnn_char_prime's loop; rnn_amd_run_text with skip >= len - 1)
 *     then exactly rnn_amd_sample_texts's loop with first = prompts[k][prompt_lens[k] - 1]: up to max_len symbols, each
 *         drawn from head `head` of alphabet_len outputs, sharpened by `bias`, ending after it has written stop_point
 * A stop symbol inside a prompt ends nothing.  Only the continuation is written to `out`, not the prompt; out_lens and
 * rng_out mean what they mean for rnn_amd_sample_texts, and what is said there about draws within rounding of a boundary
 * holds here.  `net` itself -- host and device copies, hidden row, generator -- is left exactly as it was.
 * The rows run side by side, ordered by prompt_lens[k] + max_len, longest first, in waves of up to 256 (the layout of
 * rnn_amd_run_texts): a row takes part in prompt_lens[k] + max_len - 1 forward passes, whose row count falls as the
 * shorter rows end; one launch between two passes feeds a row its next prompt symbol or draws for it.  One device
 * synchronisation per wave and one more every 64 steps, to end a wave whose every running row has met its stop symbol.
 * With one-symbol prompts the call is rnn_amd_sample_texts(first[k] = prompts[k][0]), bit for bit.
 * The prompt is not scored, every row starts from net's one hidden row and no row's state is handed back: for those
 * see rnn_amd_run_texts_from and rnn_amd_continue_texts_from below.
 * Returns 0; n_texts == 0 or max_len == 0 returns 0 at once (lengths zeroed, rng_out[k] as seeded, no device asked for).
 * Returns -1 when a row's draw met the attempt cap, as rnn_amd_sample_texts does.  Returns -1 with a message on stderr and
 * nothing computed, before anything needs a device: all that rnn_amd_sample_texts refuses; a NULL prompts or prompt_lens;
 * a prompt_lens[k] < 1 or a NULL prompts[k]; a prompt symbol outside [0, input_size) at any position; a
 * prompt_lens[k] + max_len that does not fit an int. */
int rnn_amd_continue_texts(RecurNN *net, const u8 *const *prompts, const int *prompt_lens, const u64 *seeds, int n_texts,
                           int max_len, float bias, int stop_point, int alphabet_len, int head,
                           u8 *out /* [n_texts][max_len] */, int *out_lens, rand_ctx *rng_out /* [n_texts] or NULL */);
/* The batched text calls with a STATE PER TEXT, taken from the caller and handed back: what lets them be composed -- a
 * long text scored or traced in windows, a passage drawn in instalments, a prompt scored and then continued without
 * feeding it twice -- as the reference composes rnn_char_prime, rnn_char_confabulate and more of either on one net that
 * keeps its state.  Nothing new is owned or freed: states travel through host arrays of the caller's.
 * A state is a row of net->h_size floats laid out as net->hidden_layer is.  Only its elements [1, hidden_size] carry
 * information (the input row of a forward pass takes no other, recur-nn.c:104-112).  h_in and h_out are
 * [n_texts][net->h_size], contiguous, in the caller's order.  Element 0 and the padding behind hidden_size are never read
 * from h_in; what is written there in h_out is unspecified.  Values in h_in are not inspected.
 *   h_in == NULL    every row starts from net's hidden row at the moment of the call, as in the calls above.  With h_in,
 *                   h_out (and rng_in) all NULL each call IS its counterpart above, bit for bit: rnn_amd_run_texts_from
 *                   with alphabet_len == 0 is rnn_amd_run_texts, with alphabet_len > 0 rnn_amd_run_texts_heads (sums
 *                   [n_texts][n_heads]); rnn_amd_trace_texts_from is rnn_amd_trace_texts; rnn_amd_continue_texts_from is
 *                   rnn_amd_continue_texts.
 *   h_in != NULL    clone c_k starts from h_in[k] instead.  Nothing else of those contracts changes: the texts do not see
 *                   one another, there is no noise, net's generator is untouched, and `net` -- host and device copies,
 *                   hidden row, generator, what it computes next -- is left exactly as it was.
 *   h_out != NULL   h_out[k] is c_k's hidden row after its last forward pass:
 *                   run and trace: after texts[k][0 .. lens[k] - 2] were fed; a text with lens[k] < 2 feeds nothing and
 *                     h_out[k] is its start state.
 *                   continue: after prompts[k] and out[k][0 .. out_lens[k] - 2] were fed.  The last symbol written is
 *                     never fed, whether it was the stop symbol or index max_len - 1.  (A row whose draw failed, return
 *                     -1, ends on an output row without a total; its state is the one that output row came from, after
 *                     every symbol written was fed, and is as little use.)
 *                   With h_in == NULL the start state that a text without a forward pass gets back is net's hidden row,
 *                   read without changing net's host or device copy.
 *   RESUMING        the next call on a state begins with the row's last symbol: texts[k] + lens[k] - 1 is where the next
 *                   window of a text starts (windows overlap by one symbol: a window of n symbols scores n - 1 steps),
 *                   and {out[k][out_lens[k] - 1]} is the one-symbol prompt that continues a passage -- with rng_in =
 *                   the rng_out of the call before, the instalments are the passage drawn in one call.
 *   ALIASING        h_out may be the same array as h_in, for an update in place.  Any other overlap is undefined.
 *   rng_in          (continue only) non-NULL: c_k's generator starts as rng_in[k], seeds is ignored and may be NULL.
 *                   NULL: init_rand64(seeds[k]) as above.  Both NULL with n_texts > 0 is refused.  rng_out may be rng_in.
 *   sums == NULL    allowed in rnn_amd_run_texts_from when h_out is not NULL: the texts are fed and nothing is scored,
 *                   the batched rnn_char_prime.  Both NULL with n_texts > 0 is refused.
 * Chunks and bits: two calls give the same bits where every forward pass runs in the same form (fwd_plan.h goes by the
 * row count); texts of equal lengths cut at equal places do, ragged ones agree to rounding -- the bar, not the bits, as
 * between any two calls with different row counts.  The same holds for a row that has met its stop symbol inside the
 * running prefix of its wave: it is not fed again and the later passes recompute its hidden row from the same input row,
 * so between calls whose other rows differ its h_out is equal to rounding, not to the bit.
 * Cost: one host-to-device copy of a wave's states before its first launch and one back in front of the wave's one
 * synchronisation, h_size floats per row each; no synchronisation is added.
 * Returns as the counterparts do, and: n_texts == 0 returns 0 and touches nothing; max_len == 0 in continue zeroes the
 * lengths, rng_out[k] is the start generator and h_out[k] the start state; where no text takes a row (every lens[k] < 2,
 * or max_len == 0) and h_in is given, h_out is filled by the host alone and no device is asked for.  Returns -1 with a
 * message on stderr and nothing computed, before anything needs a device: all that the counterpart refuses, and the two
 * refusals above.  There is no _from form of rnn_amd_sample_texts: a one-symbol prompt is that call, bit for bit. */
int rnn_amd_run_texts_from(RecurNN *net, const u8 *const *texts, const int *lens, const int *skips, int n_texts,
                           int alphabet_len, const float *h_in, float *h_out, double *sums);
int rnn_amd_trace_texts_from(RecurNN *net, const u8 *const *texts, const int *lens, int n_texts, int alphabet_len,
                             const float *h_in, float *h_out, float *const *logp, u8 *const *guess);
int rnn_amd_continue_texts_from(RecurNN *net, const u8 *const *prompts, const int *prompt_lens, const u64 *seeds,
                                const rand_ctx *rng_in, int n_texts, int max_len, float bias, int stop_point,
                                int alphabet_len, int head, const float *h_in, float *h_out,
                                u8 *out /* [n_texts][max_len] */, int *out_lens, rand_ctx *rng_out /* [n_texts] or NULL */);
/* Many DENSE FEATURE SEQUENCES against one net in one batched device run: using a trained classifier, as the batched
 * text calls use a trained character model.  Sequence k is n_frames[k] rows of net->input_size floats at inputs[k], row
 * stride ld_inputs floats.  What is written for it is what this loop writes on a forward-only clone c_k of `net`
 * (emit_opinions' loop body, gstclassify.c:2259-2292, for one channel):
 *     for every frame t: answer = rnn_opinion(c_k, inputs[k] + t * ld_inputs, 0);
 *         for every class group g: winners[k][t * n_groups + g] =
 *             softmax_best_guess(error + group_offset[g], answer + group_offset[g], group_size[g]);
 *         answers[k][t * output_size + i] = -error[i] for a column i inside a group, answer[i] for any other
 * that is: a column inside a group gets its softmax probability within the group (badmaths.h:71-111: the shift,
 * fast_expf, the sum in index order, the division -- the number gstclassify publishes), a column in no group the raw
 * output (rnn_amd_classify_parse_classes counts the commas of the class string in its offsets, so such columns exist),
 * and with n_groups == 0 every column is rnn_opinion's answer: the plain forward run of rnnca and parrot.  A winner is the
 * index within its group of the largest probability after the division, the lowest index among equals.
 * answers[k] is [n_frames[k]][net->output_size], winners[k] is [n_frames[k]][n_groups] bytes; winners may be NULL (none
 * are taken).  answers[k], winners[k] and inputs[k] of a sequence without a frame may be NULL; nothing is written for it,
 * nor behind the entries of any other.  Every entry is written exactly once.
 * States are the _from text calls': c_k starts from net's hidden row at the moment of the call (h_in NULL) or from h_in[k],
 * a row of net->h_size floats laid out as net->hidden_layer whose elements [1, hidden_size] carry the state; h_out[k]
 * (h_out may be NULL) is c_k's hidden row after its last frame, for a sequence without a frame its start state; h_out may
 * be h_in.  A recording cut into pieces run by successive calls joined through h_out -> h_in is the recording run in one
 * call (to the bit where the passes run with the same row counts, else to rounding, as said above for the texts).
 * There is no noise and no generator is touched; `net` -- host and device copies, hidden row, what it computes next --
 * is left exactly as it was.
 * The rows go longest first in waves of up to 256 (the layout of rnn_amd_run_texts: n frames are a text of n + 1
 * symbols).  A frame costs 4 * input_size bytes, so a wave is STAGED IN SEGMENTS of at most segment_frames frames: per
 * segment one upload of the frames of the rows that still run, the launches, one copy back of the segment's answers and
 * one of its winners, one device synchronisation.  The staging buffers -- on the device and as many bytes on the host --
 * hold one segment: the sum over the first wave's rows of min(n_frames, segment_frames), times 4 * input_size bytes of
 * frames, 4 * output_size of answers and n_groups of winners.  segment_frames <= 0: the default, the largest count for
 * which 256 rows' frames stay within 2 MiB (2 MiB / (1024 * input_size), at least 1; 64 frames at 32 features).  The
 * segment size changes no bit of the result.
 * Returns 0; where no sequence has a frame it returns 0 at once (h_out filled by the host) and asks for no device.  Returns
 * -1 with a message on stderr and nothing computed, before anything needs a device: a NULL net; n_seqs, n_groups or an
 * n_frames[k] below 0; a net with a bottom layer (as rnn_amd_run_texts); a group with no class, one that leaves the
 * output row or overlaps another; ld_inputs < net->input_size; a NULL inputs, n_frames or answers with n_seqs > 0, a
 * NULL group_offset or group_size with n_groups > 0, a NULL inputs[k], answers[k] or (with winners) winners[k] for a
 * sequence with a frame; winners with n_groups == 0 or with a group of more than 256 classes. */
int rnn_amd_run_sequences(RecurNN *net, const float *const *inputs, const int *n_frames, int n_seqs, int ld_inputs,
                          int n_groups, const int *group_offset, const int *group_size, const float *h_in, float *h_out,
                          int segment_frames, float *const *answers, u8 *const *winners);
/* Many TEXTS against one CLASSIFIER net in one batched device run: using a net that text-classify trained, and its
 * validation score.  What is written for text k is what this loop writes on a forward-only clone c_k of `net`
 * (text-classify-results.c:83-122; with classes, the validation block of rnn_char_classify_epoch,
 * charmodel-classify.c:174-196):
 *     for j in 0 .. lens[k] - 1:  raw = one_hot_opinion(c_k, texts[k][j], 0)          (no noise)
 *         if j >= skips[k]:       softmax(p, raw, net->output_size)                   (all outputs as one group)
 *             for every class c:  sums[k * output_size + c] += p[c];  sumsqs[k * output_size + c] += p[c] * p[c]
 *             if classes[k] and cl = classes[k][j] is not 0xFF (charmodel.h's NO_CLASS):
 *                 scores[k].error += 1 - p[cl];  scores[k].entropy -= capped_log2f(p[cl]);
 *                 scores[k].correct += (softmax_best_guess's pick == cl);  scores[k].count += 1
 * The softmax is badmaths.h:71-111's: the shift, fast_expf, the sum in index order, the division.  The product p[c] * p[c]
 * is formed in float, as the reference forms it; every addition is in double where the reference adds in float.  The best
 * guess is the largest probability after the division, the lowest index among equals (badmaths.h:113-141).
 * Unlike the scorers (rnn_amd_run_texts), EVERY symbol is fed and, from skips[k] on, scored -- as the frames of
 * rnn_amd_run_sequences are: c_k's state ends behind the text's last symbol, and the next call simply continues with the
 * next chunk of the text (no overlap by one symbol).  sums, sumsqs and scores are SET by the call, not added to: a text
 * run in chunks is the sum of its chunks' results.
 * skips, classes, any classes[k], sumsqs and scores may be NULL (no skip; no symbol has a class; not wanted).  A text with
 * skips[k] >= lens[k] is fed and never scored; a negative skip is 0.  A text of 0 symbols takes no row: its sums and score
 * are zeros and its h_out is its start state; texts[k] and classes[k] of such a text may be NULL.
 * States are the _from text calls': c_k starts from net's hidden row at the moment of the call (h_in NULL) or from h_in[k],
 * a row of net->h_size floats laid out as net->hidden_layer whose elements [1, hidden_size] carry the state; h_out[k]
 * (h_out may be NULL, or h_in) is c_k's hidden row after its last symbol.  A text cut into pieces run by successive calls
 * joined through h_out -> h_in is the text run in one call (the states to the bit where the passes run with the same row
 * counts, else to rounding; the sums to the grouping of their double additions).
 * There is no noise and no generator is touched; `net` -- host and device copies, weights, hidden row, what it computes
 * next -- is left exactly as it was.
 * The rows go longest first in waves of up to 256 (the layout of rnn_amd_run_texts: len symbols are a scorer's text of
 * len + 1).  Texts and class bytes go up whole, a byte per symbol; per wave there is one launch between two forward
 * passes, one synchronisation, and one copy back of 2 * output_size + 4 eight-byte words per row.
 * Returns 0; n_texts == 0 returns 0 and touches nothing; where every text is empty it returns 0 at once (zeros, h_out
 * filled by the host) and asks for no device.  Returns -1 with a line on stderr and nothing computed, before anything
 * needs a device: a NULL net; n_texts < 0; a net with a bottom layer (as rnn_amd_run_texts); a NULL texts, lens or sums
 * with n_texts > 0; a lens[k] below 0; a NULL texts[k] of a text with a symbol; a symbol >= net->input_size; a class byte
 * that is neither 0xFF nor < net->output_size. */
typedef struct RnnAmdClassScore {
  double error;      /* sum of 1 - p[class]                 */
  double entropy;    /* sum of -capped_log2f(p[class])      */
  long long correct; /* symbols whose best guess == class   */
  long long count;   /* symbols that had a class            */
} RnnAmdClassScore;
int rnn_amd_classify_texts(RecurNN *net, const u8 *const *texts, const int *lens, const int *skips,
                           const u8 *const *classes, int n_texts, const float *h_in, float *h_out, double *sums,
                           double *sumsqs, RnnAmdClassScore *scores);
/* RNNCA'S AUTOMATON played on the device, many frames in one run: the batched form of fill_frame (gstrnnca.c:805-831).
 * The grid is width * height cells, cell (cx, cy) at index cy * width + cx; a frame is three planes of that many bytes
 * (Y, Cb, Cr).  Every cell is a forward-only clone of `net`.  frames[t] is what fill_frame leaves in play_frame after its
 * (t + 1)-th call, frame -1 being `seed`:
 *     for every cell: fill_net_inputs from frame t - 1 -- the luma of the cell's len_y neighbours at offsets_y, (Cb, Cr) of
 *         its len_c neighbours at offsets_c, each byte times (1.0f / 255.0f), then the position cx * 1.0f / width,
 *         cy * 1.0f / height and with len_pos == 3 a third input (gstrnnca.c:689, evaluated in double); a neighbour beyond
 *         the grid is the clamped one (edges != 0) or the one a SINGLE wrap reaches (edges == 0);
 *         answer = rnn_opinion(clone, inputs, 0); fast_sigmoid_array(answer, answer, 3)
 *     for every cell: the bytes of frame t = the truncations of answer[0 .. 2] * 255.9f
 * (a scaled value outside [0, 256), which C leaves undefined, stores 0 if it is NaN or negative and 255 otherwise).
 * rnn_amd_automaton_parse_offsets expands an offset pattern such as the default "Y00120111C0111" as setup_inputs does
 * (gstrnnca.c:375-439; the default gives 17 Y and 8 C offsets: 17 + 2 * 8 + 2 = 35 inputs) into arrays of max_pairs
 * (dx, dy) pairs each; unknown characters are skipped.  It returns 0, or -1 with a line on stderr when a list does not
 * fit (nothing is written behind the arrays) or an argument is NULL.
 * check_for_stasis (gstrnnca.c:764-802) draws from the caller's generator and may rewrite the frame: it stays with the
 * caller, between calls, on frames[last] before it becomes the next call's seed.
 * States are the _from text calls': cell k starts from net's hidden row at the moment of the call (h_in NULL) or from
 * h_in[k], a row of net->h_size floats laid out as net->hidden_layer whose elements [1, hidden_size] carry the state;
 * h_out[k] (h_out may be NULL, or h_in) is the cell's hidden row after the last frame.  A run cut into two calls, joined
 * by frames[last] as the next seed and h_out -> h_in, is the uncut run, bit for bit.  The states move in one copy each way.
 * There is no noise and no generator is touched; `net` -- host and device copies, hidden row, what it computes next --
 * is left exactly as it was.
 * All width * height rows run in lock step (there are no waves: a cell reads its neighbours), between two forward passes
 * one launch paints the frame and builds the next input rows, and the host is not visited per frame: the frames stay on
 * the device and come back in one copy with one synchronisation per SEGMENT of at most segment_frames frames
 * (segment_frames <= 0: the default, the largest count whose bytes stay within 16 MiB, at least 1; 404 frames of
 * 144 x 96).  The device buffer holds one segment.  The segment size changes no bit.
 * Returns 0; n_frames == 0 returns 0 at once, asks for no device and with h_in given copies the states to h_out on the
 * host.  Returns -1 with a line on stderr and nothing computed, before anything needs a device: a NULL net, ca or seed, or
 * NULL frames with n_frames > 0; n_frames < 0; width or height < 1 or a product beyond int; len_y or len_c < 0 or a NULL
 * list with a positive length; len_pos other than 2 or 3; net->input_size != len_y + 2 * len_c + len_pos;
 * net->output_size < 3; a net with a bottom layer (as rnn_amd_run_texts); with edges == 0 an offset with |dx| >= width or
 * |dy| >= height, which the reference's single wrap would take out of the plane. */
typedef struct RnnAmdAutomaton {
  int width, height;
  const int *offsets_y; /* (dx, dy) pairs */
  int len_y;
  const int *offsets_c;
  int len_c;
  int len_pos; /* 2 or 3 */
  int edges;   /* non-zero: clamp; 0: wrap once */
} RnnAmdAutomaton;
int rnn_amd_automaton_parse_offsets(const char *pattern, int *offsets_y, int *len_y, int *offsets_c, int *len_c,
                                    int max_pairs);
int rnn_amd_run_automaton(RecurNN *net, const RnnAmdAutomaton *ca, const u8 *seed /* [3][height * width] */, int n_frames,
                          const float *h_in, float *h_out /* [height * width][h_size] */, int segment_frames,
                          u8 *frames /* [n_frames][3][height * width] */);
/* RNNCA'S TRAINER on the device, many generations in one call (gstrnnca.c: fill_net_inputs 669-691, train_net 693-716,
 * maybe_learn 718-750).  `set` is a training set of n_nets trainers, clones of one net with bptt and no bottom layer; `ca`
 * the grid and what a cell sees of it, as above; `frames` a film of n_steps + 1 frames of bytes; xy the trainers' cells as
 * (x, y) pairs, one list for the block (xy_per_step == 0) or one per generation.  Generation t, for t = 0 .. n_steps - 1:
 *     rnn_bptt_clear_deltas
 *     for every trainer j at (x, y) = xy[t or 0][j]:
 *         rnn_bptt_advance when `advance` is not 0 (the plugin never advances its trainers' rings: advance = 0 is the
 *             plugin; advance = 1 is rnn_amd_set_advance in front of rnn_amd_set_dense_step_sigmoid_mse)
 *         inputs = fill_net_inputs from frames[t] at (x, y), by rnn_amd_run_automaton's rule bit for bit, with ca->edges as
 *             given (the plugin always trains clamped, gstrnnca.c:698: pass edges = 1 for the plugin)
 *         answer = rnn_opinion(trainer, inputs, net->presynaptic_noise); fast_sigmoid_array(answer, answer, 3)
 *         o_error[k] = a (1 - a) (target[k] - a), target[k] = frames[t + 1][k][y * width + x] * (1.0f / 255.0f), k = 0, 1, 2
 *         rnn_bptt_calc_deltas, summed over the trainers
 *     rnn_apply_learning(nets[0], learning_style, m) with m = momentum when momentum_soft_start == 0, otherwise
 *         rnn_calculate_momentum_soft_start(nets[0]->generation, momentum, momentum_soft_start), read in front of each update
 *     rnn_condition_net(nets[0]) when `condition` is not 0 (gstrnnca.c:739)
 * that is: the results of rnn_amd_set_dense_step_sigmoid_mse on rows a host gathered by the same rule
 * (csrc/automaton_train_rule.h), bit for bit, plus STATISTICS: per trainer-generation the sum over the three outputs of
 * (target - a)^2 is added to `error` and 1 to `count` of rnn_amd_set_read_stats, so error / (3 * count) is the mean
 * squared error.  The order of that sum is the library's own: held to a float64 restatement at 1e-4 relative, as parrot's.
 * Only this call adds them: rnn_amd_set_sigmoid_mse_error, rnn_amd_set_opinion_sigmoid_mse and
 * rnn_amd_set_dense_step_sigmoid_mse leave the statistics alone.  OUTPUTS THAT ARE NOT FINITE follow the sigmoid loss's
 * rule ("OUTPUTS THAT ARE NOT FINITE" above), elementwise, and every call returns.
 * The film, the positions and the offset lists go up once per block, into a buffer of the engine's that grows on demand
 * and is freed with the engine; ONE launch gathers every generation's input and target rows from the film's bytes; the
 * generations read them where they lie.  There is no upload and no synchronisation per generation (the block's own upload
 * is waited for where it does not fit the mailbox; the conditioning's random damage, where the net's flags ask for it,
 * draws on the host).  The last frame of a block is the first of the next: a caller chains blocks.  The positions are the
 * caller's -- the plugin moves one trainer every 8 generations (gstrnnca.c:743-748), which xy_per_step expresses --, and
 * the call draws from no generator beyond what the generations themselves draw.  What is not emulated: the plugin's
 * choice of positions and its stasis check, which stay with the caller.
 * It aborts with a message (which blocks it takes is stated once, csrc/automaton_train_rule.h: automaton_block_refusal,
 * tested there without a device) on: a NULL set, ca, frames or xy; n_steps < 1; everything rnn_amd_run_automaton refuses
 * about the grid, the lists, len_pos, the net's inputs and outputs and a wrapped offset; a set with a bottom layer; any
 * (x, y) outside the grid -- every entry of xy is checked on the host before anything is launched. */
void rnn_amd_set_automaton_steps(RnnAmdSet *set, const RnnAmdAutomaton *ca,
                                 const u8 *frames /* [n_steps + 1][3][height * width] */,
                                 const int *xy /* [xy_per_step ? n_steps : 1][n_nets][2]: (x, y) */, int xy_per_step,
                                 int n_steps, int advance, int learning_style, float momentum, float momentum_soft_start,
                                 int condition);
/* GSTCLASSIFY'S TRAINER on the device, many windows in one call (gstclassify.c: train_channel 2070-2127, maybe_learn
 * 2180-2257).  `set` is a training set whose streams are the audio channels; features[t][j] is channel j's feature row of
 * window t (input_size floats, rows ld apart), targets[t][j][i] its class in group i -- < 0 or >= group_size[i]: no label.
 * The outputs are n_groups class groups, group i the columns group_offset[i] .. + group_size[i] - 1; error_weight (or
 * NULL) one factor per output.  Generation t, for t = 0 .. n_steps - 1, is maybe_learn's body:
 *     rnn_bptt_clear_deltas
 *     for every channel j: rnn_opinion(features[t][j]); the class-group loss against targets[t][j] (softmax per labelled
 *         group, +1 on the target, zeros in the groups without a label, the whole row times error_weight where any group
 *         is labelled); rnn_bptt_calc_deltas, summed, for the channels that have a label; rnn_bptt_advance behind them
 *     if (err_sum) rnn_apply_learning(nets[0], learning_style,
 *                      rnn_calculate_momentum_soft_start(nets[0]->generation, nets[0]->bptt->momentum, momentum_soft_start))
 *     rnn_condition_net(nets[0]) when `condition` is not 0
 * THE UPDATE GATE is the reference's `if (err_sum)`, exactly and without a read-back: err_sum is the sum of the trained
 * groups' wrongness 1 - p[target], every term >= 0, so it is non-zero iff some trained channel's wrongness is not 0.0f (a
 * NaN counts as non-zero); the loss kernel raises a word on the device and the optimiser launch reads it
 * (csrc/classify_train_rule.h states the rule and why it is the reference's).  A classifier that has become certain --
 * every trained group's likelihood exactly 1 -- therefore makes NO update, not a momentum-only one.  A generation in which
 * no channel has a label makes no delta call and no update.  After a generation whose gate stayed closed the weights,
 * momentum and aux arrays are what they were; the delta arrays hold that generation's sums all the same; the statistics
 * (rnn_amd_set_read_stats: error, correct, count) hold the loop's figures; the channels' generation counters have stepped.
 * The results are those of a loop of rnn_amd_classify_generation(..., balance NULL, exact_gate 1) over the windows, bit
 * for bit (that loop decides its gate from the statistics it reads back: clear them first where the difference of two
 * large sums could lose a small error).
 * Features, targets, every generation's mask of labelled channels (each on a 4-byte boundary), n_steps gate words, the
 * groups and the weights go up once per block, into a buffer of the engine's that grows on demand and is freed with the
 * engine; the generations read them where they lie: no upload per generation, no synchronisation between generations
 * (the block's own upload is waited for where it does not fit the mailbox; the conditioning's random damage, where the
 * net's flags ask for it, draws on the host).  Output layer, loss and top backprop are ONE launch exactly where
 * rnn_amd_set_opinion_grouped_softmax makes them one -- at most 64 output columns and a whole number of 4 channels --,
 * otherwise the forward pass and the loss kernel: the two forms sum the output layer in different orders, and the block
 * keeps the loop's bits at every set size.  Both read the block, and the delta call reads the generation's mask there
 * whatever the number of channels.  The update is always a launch of its own, never the delta GEMM's epilogue.
 * A set with a bottom layer, a net with presynaptic noise, a joined exchange (rnn_amd_set_exchange_join) and a distributed
 * group of more than one rank run generation by generation from the host rows instead, the gate read back: same results.
 * It aborts with a message (which blocks it takes is stated once, csrc/classify_train_rule.h: classify_block_refusal,
 * tested there without a device) on: NULL features or targets; n_steps < 1; ld < input_size; n_groups < 1 or no group
 * lists; a group that is empty or not within the outputs; a forward-only set. */
void rnn_amd_set_classify_steps(RnnAmdSet *set, const float *features /* [n_steps][n_nets][ld] */, int ld,
                                const int *targets /* [n_steps][n_nets][n_groups], <0 or >=size: not trained */,
                                int n_steps, int n_groups, const int *group_offset, const int *group_size,
                                const float *error_weight, int learning_style, float momentum_soft_start, int condition);
/* PARROT'S PLAYER on the device, many closed-loop sequences in one run: the batched form of fill_audio_chunk's loop over
 * the channels (gstparrot.c:556-583), in which every channel's dream net is fed its own last answer.  Sequence k is a
 * forward-only clone c_k of `net` with a generator g_k and an input row x_k = first[k] (net->input_size floats, row stride
 * ld_first):
 *     for t in 0 .. n_frames - 1:
 *         raw = rnn_opinion(c_k, x_k, 0)                                          (no presynaptic noise)
 *         a[i] = fast_tanhf(raw[i]);  frames[t][k][i] = a[i]                      for every output i
 *         x_k[i] = a[i] * (1.0f + noise * cheap_gaussian_noise(g_k))              for i = 0 .. output_size - 1, in index order
 *     next[k] = x_k;  rng_out[k] = g_k;  h_out[k] = c_k's hidden row
 * The answer is the next input, so net->input_size == net->output_size is required.  fast_tanhf is badmaths.h:55-68:
 * -1.0f at x <= -4.97f, 1.0f at x >= 4.97f, else x * (135135 + x2 * (17325 + x2 * (378 + x2))) divided by
 * 135135 + x2 * (62370 + x2 * (3150 + x2 * 28)), x2 = x * x, every operation one fp32 rounding; NaN stays NaN.  The noise
 * product is rounded, then the sum, then the product with a[i] -- never a + a * g; with noise == 1.0f the line is
 * gstparrot.c:576 to the bit.  The emergency soft clip of an input row (maybe_scale_inputs, recur-nn.c:68-81) belongs to
 * rnn_opinion: x_k and next[k] are the values before it.
 *   generators     g_k starts as rng_in[k], or with rng_in == NULL as init_rand64(seeds[k]): the continuer's _from
 *                  convention.  rng_out may be NULL, or rng_in.
 *   noise == 0.0f  nothing is drawn and no generator is touched: seeds and rng_in may both be NULL, next[k] is the last
 *                  frame, and rng_out[k] is the start generator where the call names one (else it is not written).
 *   states         exactly the _from calls': c_k starts from net's hidden row at the moment of the call (h_in NULL) or
 *                  from h_in[k], a row of net->h_size floats laid out as net->hidden_layer whose elements
 *                  [1, hidden_size] carry the state; h_out (NULL, or h_in) gets the hidden rows after the last frame.
 *   cutting a run  a run cut into two calls, joined through next -> first (ld_first = input_size), h_out -> h_in and
 *                  rng_out -> rng_in, is the uncut run bit for bit.
 *   net            its host and device copies, hidden row and own generator are left exactly as they were.
 *   the reference  one channel, with rng_in a copy of the shared generator and first the dream net's output row, is
 *                  fill_audio_chunk's `answer` sequence.  Many channels differ from the reference only in that each has
 *                  a generator of its own: the reference's single shared one serialises the channels.  MDCT synthesis,
 *                  overlap-add and the s16 output (gstparrot.c:568-575) stay with the caller, on `frames`.
 * All n_seqs rows run in lock step (there are no waves), between two forward passes one launch emits the frame and builds
 * the next input rows -- the draws are made on the device too, on a second stream beside the forward passes, two frames
 * ahead -- and the host is not visited per frame: the frames stay
 * on the device and come back in one copy straight into `frames` with one synchronisation per SEGMENT of at most
 * segment_frames frames (segment_frames <= 0: the default, the largest count whose floats stay within 16 MiB, at least 1;
 * 64 frames of 256 channels of 256 bins).  The device buffer holds one segment.  The segment size changes no bit.  States,
 * first, next and the generators each move in one copy each way.
 * Returns 0; n_seqs == 0 or n_frames == 0 returns 0 at once and asks for no device: next = first, rng_out = the start
 * generators and h_out = the start states are filled by the host.  Returns -1 with a line on stderr and nothing computed,
 * before anything needs a device: a NULL net; n_seqs or n_frames < 0; net->input_size != net->output_size;
 * ld_first < net->input_size; a net with a bottom layer (as rnn_amd_run_texts); a noise that is not finite; with
 * n_seqs > 0, noise != 0 with both seeds and rng_in NULL, and with n_frames > 0 as well a NULL first or frames. */
int rnn_amd_dream_sequences(RecurNN *net, const float *first /* [n_seqs][ld_first] */, int ld_first, int n_seqs,
                            int n_frames, float noise, const u64 *seeds, const rand_ctx *rng_in, const float *h_in,
                            float *h_out, int segment_frames, float *frames /* [n_frames][n_seqs][output_size] */,
                            float *next /* [n_seqs][input_size] or NULL */, rand_ctx *rng_out /* [n_seqs] or NULL */);
/* Block until all queued device work of the library has finished. */
void rnn_amd_synchronize(void);

/* Timing hook for bench.py: HIP-event time (ms) accumulated over the dominant
 * kernel class since the last reset, and the number of launches.
 * which: 0 = BPTT chain GEMM, 1 = delta GEMM, 2 = forward GEMM, 3 = optimiser, 4 = other launches,
 * 5 = the exchange step between ranks (the RCCL all-reduce of a generation, or the kernel-issued exchange's two
 * arrivals and sharded update: what a rank waits and works for between its deltas and its next forward pass). */
void rnn_amd_kernel_time_enable(int enable);
double rnn_amd_kernel_time_ms(int which, long *launches, int reset);
/* How many text steps of this process took the forward pass and the top layer as ONE launch (the north star's shape;
 * RECUR_AMD_FWD_TOP=0 for the two launches): for tests that compare the two forms. */
long rnn_amd_fwd_top_launches(void);
/* How many launches of the one-launch BPTT chain in this process started each half-step's multiply while the previous
 * half-step's row stores drained (hidden 1024, 32-stream row tiles; RECUR_AMD_CHAIN_EARLY=0 for the form without): for tests
 * that compare the two forms, which compute the same bits. */
long rnn_amd_chain_early_launches(void);

#ifdef __cplusplus
}
#endif
#endif
