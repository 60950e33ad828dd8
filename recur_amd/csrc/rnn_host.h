/* rnn_host.h -- private declarations shared by the gnu11 C host files. */
#ifndef RNN_HOST_H
#define RNN_HOST_H 1
#define _GNU_SOURCE 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include "recur_amd.h"
#include "ramd_internal.h"
#include "noise_ahead.h"

#define RAMD_MAGIC 0x444d4152u /* "RAMD" */
#define RAMD_HDR_FLOATS 16     /* 64-byte private header in front of net->mem */

#define RAMD_MIN(a, b) (((a) < (b)) ? (a) : (b))
#define RAMD_MAX(a, b) (((a) >= (b)) ? (a) : (b))

struct RamdEngine;

/* noise_ahead.c's device side of noise_ahead.h's two slots: [Scap][H] values and [Scap] generator states each, the
 * event that says slot k is filled (done[k]) and the one that orders the side stream's launches behind the main stream's
 * work (go); all made on first use */
typedef struct RamdNoiseAheadDev {
  float *noise[2];
  void *states[2];
  void *done[2]; /* hipEvent_t */
  void *go;      /* hipEvent_t */
} RamdNoiseAheadDev;

/* Lives in the first 64 bytes of the block net->mem points at.  The public
 * struct has no spare field (its layout is ABI), and no caller of the
 * reference touches net->mem (it only exists for free()). */
typedef struct RamdPriv {
  uint32_t magic;
  int stream; /* training-stream row in the engine, or -1 */
  int fwd;    /* forward-only row, or -1                   */
  int host_valid, dev_valid; /* this stream's state (RNN_AMD_STREAM) */
  struct RamdEngine *eng;
} RamdPriv;

/* One engine per set of weights: the device image of everything that the
 * nets sharing those weights own between them. */
typedef struct RamdEngine {
  struct RamdEngine *next;
  RecurNN *owner; /* the net whose ih_weights/ho_weights these are */
  RamdShape sh;
  RamdBuffers b;
  size_t ih_size, ho_size;
  int n_streams, cap_streams;
  RecurNN **streams;
  int n_fwd, cap_fwd;
  RecurNN **fwd;
  /* forward-only state rows of the engine's own, behind the clones' (rows Scap + n_fwd ...): where rnn_amd_run_texts
   * runs its batch.  The widest batch so far; the device image keeps room for that many (ramd_engine_ensure_device) */
  int scratch_fwd;
  int dev_ready;
  /* coherence of the engine-level array classes (RNN_AMD_WEIGHTS, _MOMENTUMS,
   * _DELTAS): bit set = that copy is current */
  int host_valid, dev_valid;
  int has_momentum, has_aux, has_delta;
  /* device scratch */
  void *d_scratch;      /* 256 (value,index) pairs for tall poppy + ranges */
  int *d_ranges;        /* up to 64 (start,len) pairs                       */
  int *d_mranges;       /* [Scap][65] pairs: one range list per stream (multi-head loss) */
  int *d_mclass;        /* [Scap] each stream's own class head                */
  void *d_group;        /* staging of the class-group loss: offsets, sizes, targets, weights */
  size_t d_group_bytes;
  float *d_dense;       /* staging for dense inputs, [Scap+Fcap][input_size] */
  /* the block a many-generation trainer call keeps on the device (rnn_amd_set_dense_steps_tanh's frames,
   * rnn_amd_set_automaton_steps's film and gathered rows, rnn_amd_set_classify_steps's windows): ONE buffer for all of
   * them, grown on demand (ramd_block_room) */
  void *d_block;
  size_t d_block_bytes;
  float *delta_own;     /* library-owned ih_delta||ho_delta                */
  int delta_external;
  /* The delta sums of the last set call, kept as the un-summed planes the GEMM left (in a workspace of their own)
   * for the rnn_apply_learning that normally follows to sum on its way -- the separate calls then cost what the
   * one-call text step costs, a k_delta_finalize launch less.  Whoever else wants the delta arrays gets them summed
   * first (ramd_deltas_materialize). */
  u8 *active_host; /* what b.active holds (the last active mask sent), or NULL */
  int active_host_n;
  /* the top layer's backprop of these rows has been done with the loss (rnn_amd_set_opinion_sigmoid_mse /
   * _grouped_softmax): the next rnn_amd_set_calc_deltas over them skips it -- unless anything touched the weights, the
   * hidden rows or the output error in between (ramd_top_done_clear); masked: only for the active flags in active_host */
  int top_done, top_done_row0, top_done_n, top_done_masked;
  u8 *top_done_mask; /* masked: the streams whose backprop was done (the loss's `trained` flags) */
  RamdPendingDelta kept;
  int kept_live;
  float *d_kept_slab;
  size_t kept_floats;
  /* h_error/i_error images are rebuilt lazily from ehi */
  int err_pending, err_row0, err_nrows;
  /* last per-stream scalars pushed to the device */
  float *lr_pushed;
  int *idx_pushed;
  /* rnn_bptt_clear_deltas was called and nothing has needed the zeros yet: an accumulating
   * calc_deltas that follows simply does not accumulate (ramd_deltas_materialize otherwise) */
  int deltas_zero_pending;
  /* presynaptic noise generated ahead of its forward pass: whether a pass may take it (noise_ahead.h, the rule), and
   * the two slots' device buffers and hand-over events (noise_ahead.c) */
  NoiseAhead ahead;
  RamdNoiseAheadDev ahead_dev;
  int scalars_dev_valid; /* device mef/ih_scale newer than the host structs */
  /* this engine hosts ONE SHARD of a training set spread over the ranks of the process group
   * (rnn_amd_new_training_set_shard, rnn_amd_set_shard, or a training set opened after
   * rnn_amd_dist_init): only then are the replicated host draws (weight noise, perforation,
   * random damage) a collective that takes rank 0's generator (ramd_shared_rng) */
  int sharded;
  int sharded_sets, sharded_sticky; /* open sets that shard the engine's streams; sharded for good (rnn_amd_set_shard, the shard constructor): sharded = sticky || sets > 0 */
  int mheads_alen; /* symbols per head of the last multi-head loss (0: none yet) */
  /* the exchange step as kernel-issued peer traffic (rnn_amd_set_exchange_join): every rank's delta and weight
   * arrays as device pointers valid HERE (own ones at index xchg_rank), the shared arrival counters */
  int xchg_world, xchg_rank, xchg_lockstep;
  float *xchg_delta[8], *xchg_ihw[8], *xchg_how[8];
  void *xchg_opened[8][3];   /* what hipIpcOpenMemHandle returned (to close), NULL for same-process peers */
  unsigned *xchg_flags_dev;  /* the callers' shared host counters, mapped                                  */
  void *xchg_flags_host;
  unsigned xchg_seq;
} RamdEngine;

struct RnnAmdSet {
  RamdEngine *eng;
  RecurNN **nets;
  int n;
  int row0;     /* first training-stream row, or first forward-only index when fwd_only */
  int fwd_only; /* the set is made of forward-only clones (no bptt): opinion calls only */
  int global_first, global_count;
  int counts_shard;   /* this set made the engine's streams a shard when it was opened (RamdEngine.sharded_sets counts it) */
};

static inline RamdPriv *ramd_priv(const RecurNN *net) {
  RamdPriv *p = (RamdPriv *)net->mem;
  if (!p || p->magic != RAMD_MAGIC) {
    fprintf(stderr, "librecur_amd: RecurNN %p was not created by this library\n", (void *)net);
    abort();
  }
  return p;
}

/* the rows' top backprop is no longer the one that was done with the loss (RamdEngine.top_done) */
static inline void ramd_top_done_clear(RamdEngine *e) { e->top_done = 0; }
/* ... and it has just been done with the loss, for rows [row0, row0 + n); masked: for the streams of top_done_mask only */
static inline void ramd_top_done_set(RamdEngine *e, int row0, int n, int masked) {
  e->top_done = 1;
  e->top_done_row0 = row0;
  e->top_done_n = n;
  e->top_done_masked = masked;
}

/* The host files that call the HIP runtime themselves (engine.c, net_api.c, set_api.c, set_loss.c, set_train.c,
 * noise_ahead.c, exchange.c) define RAMD_HIP_HOST before they include this header. */
#ifdef RAMD_HIP_HOST
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#define HIP_OK(x)                                                                  \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) {                                                        \
      fprintf(stderr, "librecur_amd: HIP error \"%s\" at %s:%d\n", hipGetErrorString(e_), \
              __FILE__, __LINE__);                                                 \
      abort();                                                                     \
    }                                                                              \
  } while (0)

extern hipStream_t ramd_stream;        /* engine.c: the library's stream (rnn_amd_use_device) */
extern hipStream_t ramd_side_stream;   /* noise_ahead.c: the stream the noise is generated ahead on, or NULL */
hipStream_t ramd_side_stream_ensure(void); /* noise_ahead.c: that stream, made at its first use */
extern hipEvent_t ramd_half_summed[2]; /* exchange.c: a half's sum over the ranks has arrived (ramd_delta_half_ready) */
#endif

/* engine.c: the device, the mailbox, the engines and the coherence between host and device */
void ramd_require_device(const char *what);
void *ramd_zalloc(size_t bytes);
void *ramd_dev_alloc(size_t bytes);
void ramd_dev_free(void *p);
void ramd_h2d(void *d, const void *h, size_t bytes);
void ramd_d2h(void *h, const void *d, size_t bytes);
void ramd_dsync(void);
void ramd_mail_in(void *dev, const void *host, size_t bytes);
void ramd_mail_in_flush(void);
void ramd_mail_out(void *host, const void *dev, size_t bytes);
void ramd_mail_out_flush(void);
void ramd_upload_rows_q(void *dev, const void *host, size_t host_pitch, size_t width, size_t rows, int flush);
void ramd_upload_rows(void *dev, const void *host, size_t host_pitch, size_t width, size_t rows);
void ramd_upload(void *dev, const void *host, size_t bytes);
void ramd_upload_q(void *dev, const void *host, size_t bytes);
RamdEngine *ramd_engine_new(RecurNN *owner);
void ramd_engine_delete(RamdEngine *e);
void ramd_engine_attach(RamdEngine *e, RecurNN *net);
RamdEngine *ramd_engine_of(RecurNN *net);
void ramd_engine_ensure_device(RamdEngine *e);
int ramd_state_row(const RamdEngine *e, const RamdPriv *p);
void ramd_rng_written_from_host(RamdEngine *e);
void ramd_stream_copy(RamdEngine *e, RecurNN *net, int to_device);
void ramd_stream_need_host(RamdEngine *e, RecurNN *net);
void ramd_stream_need_dev(RamdEngine *e, RecurNN *net);
void ramd_err_flush(RamdEngine *e);
void ramd_err_after_calc(RamdEngine *e, int row0, int nrows);
void ramd_deltas_materialize(RamdEngine *e);
void ramd_engine_need_host(RamdEngine *e, int what);
void ramd_engine_need_dev(RamdEngine *e, int what);
void ramd_engine_dev_wrote(RamdEngine *e, int what);
void ramd_need_host(RecurNN *net, int what);
void ramd_host_wrote(RecurNN *net, int what);
void ramd_rng_to_host(RecurNN *net);
void ramd_rng_from_host(RecurNN *net);
void *ramd_block_room(RamdEngine *e, size_t bytes);
/* carving such a block into pieces: the offset of `bytes` more behind *at, which moves on to the next 256-byte boundary */
static inline size_t ramd_block_carve(size_t *at, size_t bytes) {
  const size_t here = *at;
  *at = (here + bytes + 255) & ~(size_t)255;
  return here;
}

/* net_api.c: what the batched calls share with the per-net calls */
void ramd_host_advance(RecurNN *net);
void ramd_push_learn_rates(RamdEngine *e, int row0, int nrows);
void ramd_push_indices(RamdEngine *e, int row0, int nrows);
void ramd_pull_scalars(RamdEngine *e, int row0, int nrows);
void ramd_set_uniform_idx(RamdEngine *e, int row0, int nrows);
const int *ramd_push_ranges(RamdEngine *e, RecurErrorRange *ranges);
void ramd_log_bptt(RamdEngine *e, RecurNN *net, float mef_before);
void ramd_check_method_arrays(RamdEngine *e, int method);
int ramd_update_rule(const RecurNNBPTT *bptt, int learning_style, float momentum, float *mw, float *rate, float *ho_rate);
void ramd_apply_learning(RecurNN *net, int learning_method, float momentum, const RamdPendingDelta *pend,
                         const unsigned *gate);
void ramd_fused_net_update(RamdEngine *e, RecurNN *net, int row, unsigned batch_size);

/* texts_api.c: the refusals of rnn_amd_run_texts / _heads (alphabet_len 0: no heads), which need no device: -1 with a
 * message on stderr, else 0 */
int ramd_run_texts_refused(const char *who, const RecurNN *net, const u8 *const *texts, const int *lens, int n_texts,
                           int alphabet_len, const void *out);

/* rows_host.c: what the batched calls on forward-only state rows share (texts_api.c, sample_api.c, seqs_api.c,
 * classify_texts_api.c, automaton_api.c, dream_api.c) */
/* what all of them refuse about the net, without a device: a bottom layer, heads that do not divide the output row
 * (alphabet_len 0: no heads).  -1 with a message on stderr, else 0 */
int ramd_texts_net_refused(const char *who, const RecurNN *net, int alphabet_len);
/* net's hidden row as it stands, into row[h_size], with neither of net's copies changed; and h_out of the texts that
 * take no row (lens[k] < 2; n_rows: how many take one): their start state, h_in[k] or -- h_in NULL -- that hidden row
 * (texts_states.h).  Returns 0, or -1 out of memory */
void ramd_texts_net_hidden_row(RecurNN *net, float *row);
int ramd_texts_fill_rowless(RecurNN *net, const int *lens, int n_texts, int n_rows, const float *h_in, float *h_out);
/* One call's forward-only rows, behind the returns that ask for no device.  ramd_rows_open: the engine's image has room
 * for `widest` scratch rows, the weights and net's own state are current on the device, and the rows have no ring
 * position; e, r0 (the state row of the call's row 0), hid0 (net's hidden row on the device) and states (the rows'
 * hidden rows, contiguous from r0 on) are set.  ramd_rows_host / _dev: a zeroed staging buffer of the call's on that
 * side, at most RAMD_ROWS_STAGING a side (more aborts); ramd_rows_close frees them all. */
#define RAMD_ROWS_STAGING 8
typedef struct RamdRows {
  RamdEngine *e;
  int r0;
  const float *hid0;
  float *states;
  void *host[RAMD_ROWS_STAGING], *dev[RAMD_ROWS_STAGING];
  int n_host, n_dev;
} RamdRows;
void ramd_rows_open(RamdRows *rows, RecurNN *net, int widest);
void *ramd_rows_host(RamdRows *rows, size_t bytes);
void *ramd_rows_dev(RamdRows *rows, size_t bytes);
void ramd_rows_close(RamdRows *rows);
/* Where wave w of the plan starts: with h_in its rows' start states are packed into h_state ([rows][H], texts_states.h)
 * and copied into `states`, and NULL is returned -- the first launch reads them there as every later one does; without,
 * hid0 is returned and the first launch builds every input row from it.  ramd_rows_states_out issues the copy of the
 * first n state rows to dst (NULL: not wanted) in front of the wave's or segment's synchronisation; the caller unpacks
 * behind it. */
struct TextsPlan;
const float *ramd_rows_states_in(const RamdRows *rows, const struct TextsPlan *plan, int w, const float *h_in,
                                 float *h_state);
void ramd_rows_states_out(const RamdRows *rows, int n, float *dst);
/* the forward pass of the call's first nrows rows, whose input rows the launch before has built */
void ramd_rows_forward(const RamdRows *rows, int nrows);

/* set_api.c (what set_api.c, set_loss.c and set_train.c share among themselves: set_internal.h) */
void ramd_set_need_training(const RnnAmdSet *set, const char *what);

/* noise_ahead.c: the presynaptic noise of the next forward pass, generated ahead on the side stream (the decisions are
 * noise_ahead.h's, RamdEngine.ahead; the events that touch no device are called on that directly) */
/* the pass of state rows [r0, r0 + n) at `level` that the caller launches next: where it may take what was generated ahead
 * it waits for it and b.noise_spec / rng_spec / noise_spec_use say so; ramd_noise_ahead_pass_done clears them behind it */
void ramd_noise_ahead_pass(RamdEngine *e, int r0, int n, float level);
void ramd_noise_ahead_pass_done(RamdEngine *e);
int ramd_noise_ahead_adopted(const RamdEngine *e); /* the set's last pass took its noise from a slot */
/* the set's next pass may be generated for now: noise_ahead_offer's loss_classes, and its launches carried out */
void ramd_noise_ahead_offer(RnnAmdSet *set, int loss_classes);
void ramd_noise_ahead_free_device(RamdEngine *e); /* with the device image: the slots' buffers */
void ramd_noise_ahead_destroy(RamdEngine *e);     /* with the engine: the events */

/* exchange.c: the all-reduce overlapped with the weight-delta GEMM, for set_step (set_train.c) */
void ramd_delta_half_ready(void *ctx, int half, size_t first_float, size_t n_floats);
extern int ramd_halves_seen; /* bit h: half h's sum is on its way */

/* dist.c */
int ramd_dist_active(void);
void ramd_dist_bcast(void *host, size_t bytes, int root);
void ramd_dist_all_reduce_on(void *device_buffer, size_t n_floats, void *stream);
rand_ctx *ramd_shared_rng(RecurNN *net, rand_ctx *tmp);

/* rnn_init.c: Jenkins PRNG (recur-rng.h) */
uint64_t ramd_rand64(rand_ctx *x);
void ramd_init_rand64(rand_ctx *x, uint64_t seed);
void ramd_init_rand64_maybe_randomly(rand_ctx *x, uint64_t seed);
double ramd_rand_double(rand_ctx *x);
int ramd_rand_small_int(rand_ctx *x, int cap);
float ramd_cheap_gaussian_noise(rand_ctx *x);
float ramd_fast_expf(float x);

#endif
