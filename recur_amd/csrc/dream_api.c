/* dream_api.c -- parrot's player on the device, many closed-loop sequences in one run (gnu11 C): rnn_amd_dream_sequences,
 * the batched form of fill_audio_chunk's loop over the channels (gstparrot.c:556-583: tanh_opinion of the dream net on its
 * own last answer, then every element of the answer times 1 + cheap_gaussian_noise).  Every sequence gets a forward-only
 * state row of the engine's own, sequence k the row r0 + k, and a generator of its own in a buffer of the call's, as the
 * continuer's texts do (sample_api.c).  A sequence's next input is its own last answer, so nothing can be staged ahead
 * as seqs_api.c stages its frames; the rows have equal lengths, so there are no waves: all n_seqs rows run in lock step,
 * as the automaton's cells do (automaton_api.c), and between two forward passes of them there is one launch
 * (k_dream_step, kernels_rows.hip) that emits the frame just computed into the call's device frame buffer and builds
 * every row's next input row from it; the noise it multiplies in is drawn ahead of it on the side stream (DrawsAhead
 * below).  The rule itself is dream_rule.h's.  The frames stay on the device and come back a
 * segment at a time: one copy, one synchronisation.  States, first rows, last rows and generators travel in one copy each
 * way: all rows are live and lie in the caller's order, so there is nothing to permute.  The net the caller passes is
 * read -- its weights, its hidden row -- and not written; its own generator is not touched. */
#define RAMD_HIP_HOST 1
#include <limits.h>
#include <math.h>
#include "rnn_host.h"
#include "dream_rule.h"
#include "texts_states.h"

#define WHO "rnn_amd_dream_sequences"
/* the default segment: the largest count of frames whose floats stay within this (at least one frame) */
#define DREAM_SEGMENT_BYTES (16u << 20)

/* the refusals, which need no device: -1 with a line on stderr, else 0 */
static int dream_refused(const RecurNN *net, const float *first, int ld_first, int n_seqs, int n_frames, float noise,
                         const u64 *seeds, const rand_ctx *rng_in, const float *frames) {
  if (!net) {
    fprintf(stderr, "librecur_amd: " WHO ": a NULL net\n");
    return -1;
  }
  if (n_seqs < 0 || n_frames < 0) {
    fprintf(stderr, "librecur_amd: " WHO ": %d sequences of %d frames\n", n_seqs, n_frames);
    return -1;
  }
  if (net->input_size != net->output_size) {
    fprintf(stderr, "librecur_amd: " WHO ": the net has %d inputs and %d outputs: its answer is not its next input\n",
            net->input_size, net->output_size);
    return -1;
  }
  if (ld_first < net->input_size) {
    fprintf(stderr, "librecur_amd: " WHO ": rows of %d floats do not hold %d inputs\n", ld_first, net->input_size);
    return -1;
  }
  if (ramd_texts_net_refused(WHO, net, 0)) {
    return -1;
  }
  if (!isfinite(noise)) {
    fprintf(stderr, "librecur_amd: " WHO ": a noise level that is not finite\n");
    return -1;
  }
  if (n_seqs > 0 && n_frames > 0 && (!first || !frames)) {
    fprintf(stderr, "librecur_amd: " WHO ": a NULL first or frame array for %d sequences of %d frames\n", n_seqs, n_frames);
    return -1;
  }
  if (n_seqs > 0 && dream_draws(noise) && !seeds && !rng_in) {
    fprintf(stderr, "librecur_amd: " WHO ": noise and neither seeds nor generators for %d sequences\n", n_seqs);
    return -1;
  }
  return 0;
}

/* sequence k's generator before its first draw (the continuer's _from convention) */
static rand_ctx start_generator(const u64 *seeds, const rand_ctx *rng_in, int k) {
  rand_ctx g;
  if (rng_in) {
    g = rng_in[k];
  } else {
    ramd_init_rand64(&g, seeds[k]);
  }
  return g;
}

/* the generators of a call that draws nothing: as they start, where the caller has named a start */
static void generators_as_started(const u64 *seeds, const rand_ctx *rng_in, int n_seqs, rand_ctx *rng_out) {
  if (rng_out && (seeds || rng_in)) {
    for (int k = 0; k < n_seqs; k++) {
      rng_out[k] = start_generator(seeds, rng_in, k);
    }
  }
}

/* THE DRAWS, ahead of the launches that take them.  A generator is a recurrence -- 3 rand64 per value, one lane per
 * sequence whatever their number -- and frame t's draws depend on no answer, so they are made on the side stream beside
 * the forward passes, as the presynaptic noise of a training set is (noise_ahead.c), DRAWS_AHEAD frames ahead into that
 * many buffers.  Frame t's launch waits for its buffer's `drawn` event; the draws of frame t + DRAWS_AHEAD, which go
 * into the same buffer, wait for that launch's `taken` event.  The generators live in d_rng and are touched by the side
 * stream alone between the upload and the copy back, both of which the events order: per generator the order of draws is
 * the contract's, frame after frame in index order. */
#define DRAWS_AHEAD 2
typedef struct DrawsAhead {
  hipStream_t side;
  hipEvent_t go, drawn[DRAWS_AHEAD], taken[DRAWS_AHEAD];
  float *gz[DRAWS_AHEAD]; /* [n][rows] a frame's draws, value-major */
  rand_ctx *d_rng;
  int rows, n, n_frames;
} DrawsAhead;

static void draws_ahead_launch(DrawsAhead *a, size_t t) {
  if (t >= (size_t)a->n_frames) {
    return;
  }
  const int k = (int)(t % DRAWS_AHEAD);
  if (t >= DRAWS_AHEAD) { /* the buffer's last reader */
    HIP_OK(hipStreamWaitEvent(a->side, a->taken[k], 0));
  }
  ramd_launch_dream_draw(a->side, a->d_rng, a->gz[k], a->rows, a->n);
  HIP_OK(hipEventRecord(a->drawn[k], a->side));
}

/* the generators up (one copy), and the first DRAWS_AHEAD frames' draws under way behind it */
static void draws_ahead_open(DrawsAhead *a, RamdRows *rows, const u64 *seeds, const rand_ctx *rng_in, int n_seqs, int n,
                             int n_frames) {
  a->side = ramd_side_stream_ensure();
  a->rows = n_seqs;
  a->n = n;
  a->n_frames = n_frames;
  a->d_rng = ramd_rows_dev(rows, (size_t)n_seqs * sizeof(rand_ctx));
  if (rng_in) {
    ramd_h2d(a->d_rng, rng_in, (size_t)n_seqs * sizeof(rand_ctx));
  } else {
    rand_ctx *h_rng = ramd_rows_host(rows, (size_t)n_seqs * sizeof(rand_ctx));
    for (int k = 0; k < n_seqs; k++) {
      h_rng[k] = start_generator(seeds, NULL, k);
    }
    ramd_h2d(a->d_rng, h_rng, (size_t)n_seqs * sizeof(rand_ctx));
  }
  HIP_OK(hipEventCreateWithFlags(&a->go, hipEventDisableTiming));
  for (int k = 0; k < DRAWS_AHEAD; k++) {
    a->gz[k] = ramd_rows_dev(rows, (size_t)n_seqs * n * sizeof(float));
    HIP_OK(hipEventCreateWithFlags(&a->drawn[k], hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags(&a->taken[k], hipEventDisableTiming));
  }
  /* behind the main stream's work so far: the buffers' zeroing and the generators' upload */
  HIP_OK(hipEventRecord(a->go, ramd_stream));
  HIP_OK(hipStreamWaitEvent(a->side, a->go, 0));
  for (size_t t = 0; t < DRAWS_AHEAD; t++) {
    draws_ahead_launch(a, t);
  }
}

/* frame t's draws for the launch the caller enqueues next on the main stream, which waits for them */
static const float *draws_ahead_take(DrawsAhead *a, size_t t) {
  const int k = (int)(t % DRAWS_AHEAD);
  HIP_OK(hipStreamWaitEvent(ramd_stream, a->drawn[k], 0));
  return a->gz[k];
}

/* that launch is enqueued: its buffer is free behind it, for the draws of frame t + DRAWS_AHEAD */
static void draws_ahead_taken(DrawsAhead *a, size_t t) {
  HIP_OK(hipEventRecord(a->taken[t % DRAWS_AHEAD], ramd_stream));
  draws_ahead_launch(a, t + DRAWS_AHEAD);
}

/* behind the call's last synchronisation: every draw has been waited for by a launch that has finished */
static void draws_ahead_close(DrawsAhead *a) {
  HIP_OK(hipEventDestroy(a->go));
  for (int k = 0; k < DRAWS_AHEAD; k++) {
    HIP_OK(hipEventDestroy(a->drawn[k]));
    HIP_OK(hipEventDestroy(a->taken[k]));
  }
}

int rnn_amd_dream_sequences(RecurNN *net, const float *first, int ld_first, int n_seqs, int n_frames, float noise,
                            const u64 *seeds, const rand_ctx *rng_in, const float *h_in, float *h_out, int segment_frames,
                            float *frames, float *next, rand_ctx *rng_out) {
  if (dream_refused(net, first, ld_first, n_seqs, n_frames, noise, seeds, rng_in, frames)) {
    return -1;
  }
  if (n_seqs == 0) {
    return 0;
  }
  const size_t H = (size_t)net->h_size, W = (size_t)net->input_size, n = (size_t)n_seqs;
  if (n_frames == 0) { /* nothing to dream: rows, generators and states as they start, and no device is asked for */
    if (next && first) {
      for (size_t k = 0; k < n; k++) {
        memmove(next + k * W, first + k * (size_t)ld_first, W * sizeof(float));
      }
    }
    generators_as_started(seeds, rng_in, n_seqs, rng_out);
    if (h_out) {
      float *row = NULL;
      if (!h_in) {
        row = ramd_zalloc(H * sizeof(float));
        ramd_texts_net_hidden_row(net, row);
      }
      for (size_t k = 0; k < n; k++) {
        texts_state_take(h_out + k * H, h_in ? h_in + k * H : row, net->h_size, net->hidden_size);
      }
      free(row);
    }
    return 0;
  }
  const int draws = dream_draws(noise);
  const size_t frame_floats = n * W;
  size_t F = segment_frames > 0 ? (size_t)segment_frames
                                : RAMD_MAX(DREAM_SEGMENT_BYTES / (frame_floats * sizeof(float)), (size_t)1);
  F = RAMD_MIN(F, (size_t)n_frames);
  RamdRows rows;
  ramd_rows_open(&rows, net, n_seqs);
  RamdEngine *e = rows.e;
  const RamdShape *s = &e->sh;
  /* every sequence starts from the net's hidden row, or from its own state: all rows are live and lie in the caller's order */
  const float *hid0 = rows.hid0;
  if (h_in) {
    ramd_h2d(rows.states, h_in, n * s->H * sizeof(float));
    hid0 = NULL;
  }
  float *d_first = ramd_rows_dev(&rows, n * (size_t)ld_first * sizeof(float));
  float *d_frames = ramd_rows_dev(&rows, F * frame_floats * sizeof(float));
  float *d_next = ramd_rows_dev(&rows, frame_floats * sizeof(float));
  ramd_h2d(d_first, first, n * (size_t)ld_first * sizeof(float));
  DrawsAhead ahead = {0};
  if (draws) {
    draws_ahead_open(&ahead, &rows, seeds, rng_in, n_seqs, net->output_size, n_frames);
  } else {
    generators_as_started(seeds, rng_in, n_seqs, rng_out);
  }
  /* launch 0 feeds from `first`; launch t + 1 emits frame t and feeds from it, or, behind the last frame, leaves `next` */
  RamdDreamStep step = {.first = d_first, .ld_first = ld_first, .hid0 = hid0, .row0 = rows.r0, .rows = n_seqs, .noise = noise};
  ramd_launch_dream_step(ramd_stream, s, &e->b, &step);
  ramd_rows_forward(&rows, n_seqs);
  step.first = NULL;
  step.hid0 = NULL;
  size_t t0 = 0; /* the segment's first frame */
  for (size_t t = 0; t < (size_t)n_frames; t++) {
    const int last = t + 1 == (size_t)n_frames;
    const size_t slot = t - t0;
    step.emit = d_frames + slot * frame_floats;
    step.next = last ? d_next : NULL;
    step.gz = draws ? draws_ahead_take(&ahead, t) : NULL;
    ramd_launch_dream_step(ramd_stream, s, &e->b, &step);
    if (draws) {
      draws_ahead_taken(&ahead, t);
    }
    if (!last) {
      ramd_rows_forward(&rows, n_seqs);
    }
    if (slot + 1 == F || last) {
      ramd_d2h(frames + t0 * frame_floats, d_frames, (slot + 1) * frame_floats * sizeof(float));
      if (last) { /* a row's last forward pass was its hidden row's last writer; the last launch has waited for the last
                   * draws, its generator's last writer */
        ramd_rows_states_out(&rows, n_seqs, h_out);
        if (next) {
          ramd_d2h(next, d_next, frame_floats * sizeof(float));
        }
        if (draws && rng_out) {
          ramd_d2h(rng_out, ahead.d_rng, n * sizeof(rand_ctx));
        }
      }
      ramd_dsync(); /* the segment's one synchronisation */
      t0 = t + 1;
    }
  }
  if (draws) {
    draws_ahead_close(&ahead);
  }
  ramd_rows_close(&rows);
  return 0;
}
