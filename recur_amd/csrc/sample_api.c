/* sample_api.c -- many texts drawn from one net in one batched device run (gnu11 C): rnn_amd_sample_texts, the
 * generative counterpart of rnn_amd_run_texts (texts_api.c), and rnn_amd_char_confabulate_texts, its character layer.
 * Where rnn_char_confabulate (char_sampling.c) visits the host for every symbol of one net -- the output row comes back,
 * the host draws, the generator goes out again -- these give every text a forward-only state row of the engine's own and
 * a generator of its own in a buffer of the call's, and run the rows together: between two forward passes of the rows
 * there is one launch (k_texts_sample, kernels_loss.hip) that draws each row's next symbol on the device (sample_rule.h)
 * and builds the input rows of the next pass from it.  The net the caller passes is read -- its weights, its hidden row --
 * and not written.
 * rnn_amd_continue_texts and rnn_amd_char_continue_texts are the same with a prompt per row in front of the draws: the
 * rows are laid out by prompt length + max_len (texts_plan.h, as rnn_amd_run_texts lays out its texts), and the launch
 * between two forward passes (k_texts_continue) feeds a row its prompt or draws for it, as continue_rule.h says.
 * rnn_amd_continue_texts_from is that call with every row's start state and generator from the caller's arrays and its
 * final state handed back (texts_states.h: which state belongs to which row); rnn_amd_continue_texts is it with NULLs. */
#define RAMD_HIP_HOST 1
#include <limits.h>
#include "char_host.h"
#include "texts_plan.h"
#include "texts_states.h"
#include "continue_rule.h"

#define SAMPLE_CHECK_EVERY 64 /* steps between two looks at the rows' done words */

/* what both calls refuse about the net, the counts and the head; arrays_ok: none of the call's arrays is NULL */
static int sample_call_refused(const char *who, const RecurNN *net, int n_texts, int max_len, int alphabet_len, int head,
                               int arrays_ok) {
  if (!net || n_texts < 0 || max_len < 0) {
    fprintf(stderr, "librecur_amd: %s: %d texts of %d symbols\n", who, n_texts, max_len);
    return -1;
  }
  if (ramd_texts_net_refused(who, net, alphabet_len)) { /* (a bottom layer, heads that do not divide the outputs) */
    return -1;
  }
  const int n_heads = alphabet_len ? net->output_size / alphabet_len : 1;
  if (head < 0 || head >= n_heads) {
    fprintf(stderr, "librecur_amd: %s: head %d of %d\n", who, head, n_heads);
    return -1;
  }
  if (n_texts > 0 && !arrays_ok) {
    fprintf(stderr, "librecur_amd: %s: a NULL array for %d texts\n", who, n_texts);
    return -1;
  }
  return 0;
}

static int sample_texts_refused(const char *who, const RecurNN *net, const int *first, const u64 *seeds, int n_texts,
                                int max_len, int alphabet_len, int head, const void *out, const int *out_lens) {
  if (sample_call_refused(who, net, n_texts, max_len, alphabet_len, head, first && seeds && out && out_lens)) {
    return -1;
  }
  for (int k = 0; k < n_texts; k++) {
    if (first[k] < 0 || first[k] >= net->input_size) {
      fprintf(stderr, "librecur_amd: %s: text %d starts from symbol %d of %d inputs\n", who, k, first[k], net->input_size);
      return -1;
    }
  }
  return 0;
}

/* (seeds: the call's seeds, or where it takes the rows' generators from the caller, those) */
static int continue_texts_refused(const char *who, const RecurNN *net, const u8 *const *prompts, const int *prompt_lens,
                                  const void *seeds, int n_texts, int max_len, int alphabet_len, int head, const void *out,
                                  const int *out_lens) {
  if (sample_call_refused(who, net, n_texts, max_len, alphabet_len, head, prompts && prompt_lens && seeds && out && out_lens)) {
    return -1;
  }
  for (int k = 0; k < n_texts; k++) {
    if (prompt_lens[k] < 1 || !prompts[k]) {
      fprintf(stderr, "librecur_amd: %s: prompt %d has %d symbols%s\n", who, k, prompt_lens[k], prompts[k] ? "" : " and is NULL");
      return -1;
    }
    if (prompt_lens[k] > INT_MAX - max_len) {
      fprintf(stderr, "librecur_amd: %s: prompt %d: %d + %d symbols do not fit an int\n", who, k, prompt_lens[k], max_len);
      return -1;
    }
    for (int i = 0; i < prompt_lens[k]; i++) {
      if (prompts[k][i] >= net->input_size) {
        fprintf(stderr, "librecur_amd: %s: prompt %d has symbol %d of %d inputs at %d\n", who, k, prompts[k][i],
                net->input_size, i);
        return -1;
      }
    }
  }
  return 0;
}

/* nothing to draw: lengths zeroed, generators as seeded, no device asked for */
static int nothing_to_draw(const u64 *seeds, int n_texts, int *out_lens, rand_ctx *rng_out) {
  for (int k = 0; k < n_texts; k++) {
    out_lens[k] = 0;
    if (rng_out) {
      ramd_init_rand64(&rng_out[k], seeds[k]);
    }
  }
  return 0;
}

/* the device and host sides of one wave's arrays, with room for TEXTS_PLAN_WIDTH rows (or all the texts, if fewer) */
typedef struct SampleBuffers {
  int *d_first, *d_len, *d_done, *h_len, *h_done;
  rand_ctx *d_rng, *h_rng;
  u8 *d_text, *h_text;
} SampleBuffers;

/* rows [k0, k0 + n) of the call on the state rows from r0 on; returns the number of rows whose draw failed */
static int sample_wave(RamdEngine *e, const RecurNN *net, int r0, const int *first, const u64 *seeds, int k0, int n,
                       int max_len, float bias, int stop_point, int alen, int head, const SampleBuffers *sb, u8 *out,
                       int *out_lens, rand_ctx *rng_out) {
  const RamdShape *s = &e->sh;
  for (int j = 0; j < n; j++) {
    ramd_init_rand64(&sb->h_rng[j], seeds[k0 + j]);
  }
  ramd_h2d(sb->d_first, first + k0, (size_t)n * sizeof(int));
  ramd_h2d(sb->d_rng, sb->h_rng, (size_t)n * sizeof(rand_ctx));
  HIP_OK(hipMemsetAsync(sb->d_len, 0, (size_t)n * sizeof(int), ramd_stream));
  HIP_OK(hipMemsetAsync(sb->d_done, 0, (size_t)n * sizeof(int), ramd_stream));
  /* every row starts from the net's hidden row: the first launch builds the input rows from it */
  const float *hid0 = e->b.hidden + (size_t)ramd_state_row(e, ramd_priv(net)) * s->H;
  for (int t = 0; t <= max_len; t++) {
    ramd_launch_texts_sample(ramd_stream, s, &e->b, r0, n, sb->d_first, sb->d_rng, sb->d_text, sb->d_len, sb->d_done, hid0,
                             alen, head, max_len, t, stop_point, bias);
    if (t == max_len) {
      break;
    }
    if (t > 0 && t % SAMPLE_CHECK_EVERY == 0) { /* has every row met its stop symbol?  then the rest would run on nothing */
      ramd_d2h(sb->h_done, sb->d_done, (size_t)n * sizeof(int));
      ramd_dsync();
      int running = 0;
      for (int j = 0; j < n; j++) {
        running += sb->h_done[j] == 0;
      }
      if (!running) {
        break;
      }
    }
    const RamdFwdCall call = {.row0 = r0, .nrows = n, .rows_built = 1};
    ramd_launch_forward(ramd_stream, s, &e->b, &call, NULL, NULL);
  }
  ramd_d2h(sb->h_text, sb->d_text, (size_t)n * max_len);
  ramd_d2h(sb->h_len, sb->d_len, (size_t)n * sizeof(int));
  ramd_d2h(sb->h_done, sb->d_done, (size_t)n * sizeof(int));
  ramd_d2h(sb->h_rng, sb->d_rng, (size_t)n * sizeof(rand_ctx));
  ramd_dsync(); /* the wave's synchronisation */
  int failed = 0;
  for (int j = 0; j < n; j++) {
    const int len = RAMD_MIN(RAMD_MAX(sb->h_len[j], 0), max_len);
    memcpy(out + (size_t)(k0 + j) * max_len, sb->h_text + (size_t)j * max_len, (size_t)len);
    out_lens[k0 + j] = len;
    failed += sb->h_done[j] == 2;
    if (rng_out) {
      rng_out[k0 + j] = sb->h_rng[j];
    }
  }
  return failed;
}

int rnn_amd_sample_texts(RecurNN *net, const int *first, const u64 *seeds, int n_texts, int max_len, float bias,
                         int stop_point, int alphabet_len, int head, u8 *out, int *out_lens, rand_ctx *rng_out) {
  const char *who = "rnn_amd_sample_texts";
  if (sample_texts_refused(who, net, first, seeds, n_texts, max_len, alphabet_len, head, out, out_lens)) {
    return -1;
  }
  if (n_texts == 0 || max_len == 0) {
    return nothing_to_draw(seeds, n_texts, out_lens, rng_out);
  }
  const int alen = alphabet_len ? alphabet_len : net->output_size;
  RamdEngine *e = ramd_engine_of(net);
  const int widest = RAMD_MIN(n_texts, TEXTS_PLAN_WIDTH);
  if (e->scratch_fwd < widest) {
    e->scratch_fwd = widest; /* the image grows once (every net's state survives: ramd_engine_ensure_device) */
  }
  ramd_engine_ensure_device(e);
  ramd_engine_need_dev(e, RNN_AMD_WEIGHTS);
  ramd_stream_need_dev(e, net);
  ramd_set_uniform_idx(e, e->n_streams, 0); /* forward-only rows: no ring position */
  const int r0 = e->sh.Scap + e->n_fwd; /* the engine's scratch rows lie behind the clones' */
  SampleBuffers sb;
  sb.h_len = ramd_zalloc((size_t)widest * sizeof(int));
  sb.h_done = ramd_zalloc((size_t)widest * sizeof(int));
  sb.h_rng = ramd_zalloc((size_t)widest * sizeof(rand_ctx));
  sb.h_text = ramd_zalloc((size_t)widest * max_len);
  sb.d_first = ramd_dev_alloc((size_t)widest * sizeof(int));
  sb.d_len = ramd_dev_alloc((size_t)widest * sizeof(int));
  sb.d_done = ramd_dev_alloc((size_t)widest * sizeof(int));
  sb.d_rng = ramd_dev_alloc((size_t)widest * sizeof(rand_ctx));
  sb.d_text = ramd_dev_alloc((size_t)widest * max_len);
  int failed = 0;
  for (int k0 = 0; k0 < n_texts; k0 += TEXTS_PLAN_WIDTH) {
    failed += sample_wave(e, net, r0, first, seeds, k0, RAMD_MIN(n_texts - k0, TEXTS_PLAN_WIDTH), max_len, bias, stop_point,
                          alen, head, &sb, out, out_lens, rng_out);
  }
  ramd_dev_free(sb.d_first);
  ramd_dev_free(sb.d_len);
  ramd_dev_free(sb.d_done);
  ramd_dev_free(sb.d_rng);
  ramd_dev_free(sb.d_text);
  free(sb.h_len);
  free(sb.h_done);
  free(sb.h_rng);
  free(sb.h_text);
  if (failed) {
    fprintf(stderr, "librecur_amd: %s: %d of %d texts met the attempt cap of the draw (an output row without a total)\n",
            who, failed, n_texts);
    return -1;
  }
  return 0;
}

/* the device and host sides of one wave of rnn_amd_continue_texts: SampleBuffers (d_first unused) and the prompts */
typedef struct ContinueBuffers {
  SampleBuffers sb;
  u8 *h_prompt, *d_prompt;
  unsigned long long *h_off, *d_off;
  int *h_plen, *d_plen;
  float *h_state; /* [rows][H] the wave's states on their way in and out, or NULL */
} ContinueBuffers;

/* where a call's rows start and what it hands back of them besides the text: start states and generators (NULL: the
 * net's hidden row, init_rand64 of the seeds), final states and generators (NULL: not wanted) */
typedef struct ContinueStates {
  const float *h_in;
  float *h_out;
  const u64 *seeds;
  const rand_ctx *rng_in;
  rand_ctx *rng_out;
} ContinueStates;

/* row k's generator before its first draw */
static rand_ctx start_generator(const ContinueStates *cs, int k) {
  rand_ctx g;
  if (cs->rng_in) {
    g = cs->rng_in[k];
  } else {
    ramd_init_rand64(&g, cs->seeds[k]);
  }
  return g;
}

/* wave w of the plan (its len is prompt length + max_len) on the state rows from r0 on; returns the number of rows whose
 * draw failed */
static int continue_wave(RamdEngine *e, const RecurNN *net, const TextsPlan *plan, int w, int r0, const u8 *const *prompts,
                         const ContinueStates *cs, int max_len, float bias, int stop_point, int alen, int head,
                         const ContinueBuffers *cb, u8 *out, int *out_lens) {
  const RamdShape *s = &e->sh;
  const SampleBuffers *sb = &cb->sb;
  const TextsWave *wave = &plan->waves[w];
  const int n = wave->nrows;
  size_t at = 0;
  for (int j = 0; j < n; j++) {
    const int k = plan->order[wave->row0 + j], plen = plan->len[wave->row0 + j] - max_len;
    cb->h_off[j] = at;
    cb->h_plen[j] = plen;
    memcpy(cb->h_prompt + at, prompts[k], (size_t)plen);
    at += (size_t)plen;
    sb->h_rng[j] = start_generator(cs, k);
  }
  ramd_h2d(cb->d_prompt, cb->h_prompt, at);
  ramd_h2d(cb->d_off, cb->h_off, (size_t)n * sizeof(unsigned long long));
  ramd_h2d(cb->d_plen, cb->h_plen, (size_t)n * sizeof(int));
  ramd_h2d(sb->d_rng, sb->h_rng, (size_t)n * sizeof(rand_ctx));
  HIP_OK(hipMemsetAsync(sb->d_len, 0, (size_t)n * sizeof(int), ramd_stream));
  HIP_OK(hipMemsetAsync(sb->d_done, 0, (size_t)n * sizeof(int), ramd_stream));
  /* every row starts from the net's hidden row: the first launch builds the input rows from it.  Or from its own state:
   * the wave's rows of h_in go into the state rows, which are contiguous, and the first launch reads them there as every
   * later one does (a null hid0, k_texts_continue) */
  const float *hid0 = e->b.hidden + (size_t)ramd_state_row(e, ramd_priv(net)) * s->H;
  float *states = e->b.hidden + (size_t)r0 * s->H;
  if (cs->h_in) {
    texts_states_pack(plan, w, cs->h_in, NULL, s->H, s->hidden_size, cb->h_state);
    ramd_h2d(states, cb->h_state, (size_t)n * s->H * sizeof(float));
    hid0 = NULL;
  }
  const int lead = cb->h_plen[0]; /* the wave's longest row: its launches are the wave's */
  int rows = n;                   /* the rows launch t is for: those that were fed after launch t - 1 */
  for (int t = 0;; t++) {
    const ContinueStep st = continue_step(lead, max_len, t);
    if (st.what == CONTINUE_IDLE) {
      break;
    }
    ramd_launch_texts_continue(ramd_stream, s, &e->b, r0, rows, cb->d_prompt, cb->d_off, cb->d_plen, sb->d_rng, sb->d_text,
                               sb->d_len, sb->d_done, hid0, alen, head, max_len, t, stop_point, bias);
    if (!st.feeds) { /* the longest row's last draw */
      break;
    }
    const int a = texts_plan_active(plan, w, t); /* the rows that are fed after launch t: a prefix (texts_plan.h) */
    if (t > 0 && t % SAMPLE_CHECK_EVERY == 0) { /* has every such row met its stop symbol?  then the rest would run on nothing */
      ramd_d2h(sb->h_done, sb->d_done, (size_t)a * sizeof(int));
      ramd_dsync();
      int running = 0;
      for (int j = 0; j < a; j++) {
        running += sb->h_done[j] == 0;
      }
      if (!running) {
        break;
      }
    }
    const RamdFwdCall call = {.row0 = r0, .nrows = a, .rows_built = 1};
    ramd_launch_forward(ramd_stream, s, &e->b, &call, NULL, NULL);
    rows = a;
  }
  ramd_d2h(sb->h_text, sb->d_text, (size_t)n * max_len);
  ramd_d2h(sb->h_len, sb->d_len, (size_t)n * sizeof(int));
  ramd_d2h(sb->h_done, sb->d_done, (size_t)n * sizeof(int));
  ramd_d2h(sb->h_rng, sb->d_rng, (size_t)n * sizeof(rand_ctx));
  if (cs->h_out) {
    /* every row has had a forward pass (launch 0 feeds them all), and its hidden row is the one after its last feed: a
     * pass over a row that was not fed since recomputes that row from the same input row, and a look above ends the wave
     * only where its launch fed no row (every row it could have fed is done) */
    ramd_d2h(cb->h_state, states, (size_t)n * s->H * sizeof(float));
  }
  ramd_dsync(); /* the wave's synchronisation */
  if (cs->h_out) {
    texts_states_unpack(plan, w, cb->h_state, s->H, cs->h_out);
  }
  int failed = 0;
  for (int j = 0; j < n; j++) {
    const int k = plan->order[wave->row0 + j];
    const int len = RAMD_MIN(RAMD_MAX(sb->h_len[j], 0), max_len);
    memcpy(out + (size_t)k * max_len, sb->h_text + (size_t)j * max_len, (size_t)len);
    out_lens[k] = len;
    failed += sb->h_done[j] == 2;
    if (cs->rng_out) {
      cs->rng_out[k] = sb->h_rng[j];
    }
  }
  return failed;
}

static int continue_texts(const char *who, RecurNN *net, const u8 *const *prompts, const int *prompt_lens, int n_texts,
                          int max_len, float bias, int stop_point, int alphabet_len, int head, const ContinueStates *cs,
                          u8 *out, int *out_lens) {
  if (continue_texts_refused(who, net, prompts, prompt_lens, cs->rng_in ? (const void *)cs->rng_in : (const void *)cs->seeds,
                             n_texts, max_len, alphabet_len, head, out, out_lens)) {
    return -1;
  }
  if (n_texts == 0) {
    return 0;
  }
  if (max_len == 0) { /* nothing to draw: lengths zeroed, generators and states as they start, no device asked for... */
    for (int k = 0; k < n_texts; k++) {
      out_lens[k] = 0;
      if (cs->rng_out) {
        cs->rng_out[k] = start_generator(cs, k);
      }
    }
    /* (... unless the start state is the net's hidden row and only the device has it.  No text takes a row) */
    if (ramd_texts_fill_rowless(net, out_lens, n_texts, 0, cs->h_in, cs->h_out)) {
      fprintf(stderr, "librecur_amd: %s: out of memory\n", who);
      return -1;
    }
    return 0;
  }
  int *lens = ramd_zalloc((size_t)n_texts * sizeof(int)); /* what a row is planned by: the forward passes it takes, plus 1 */
  TextsPlan plan;
  for (int k = 0; k < n_texts; k++) {
    lens[k] = prompt_lens[k] + max_len; /* at least 2: every prompt takes a row */
  }
  const int unplanned = texts_plan_make(&plan, lens, NULL, n_texts, TEXTS_PLAN_WIDTH);
  free(lens);
  if (unplanned) {
    fprintf(stderr, "librecur_amd: %s: out of memory planning %d texts\n", who, n_texts);
    return -1;
  }
  const int alen = alphabet_len ? alphabet_len : net->output_size;
  RamdEngine *e = ramd_engine_of(net);
  const int widest = plan.waves[0].nrows;
  if (e->scratch_fwd < widest) {
    e->scratch_fwd = widest; /* the image grows once (every net's state survives: ramd_engine_ensure_device) */
  }
  ramd_engine_ensure_device(e);
  ramd_engine_need_dev(e, RNN_AMD_WEIGHTS);
  ramd_stream_need_dev(e, net);
  ramd_set_uniform_idx(e, e->n_streams, 0); /* forward-only rows: no ring position */
  const int r0 = e->sh.Scap + e->n_fwd; /* the engine's scratch rows lie behind the clones' */
  size_t bytes = 0; /* of the first wave's prompts: the longest rows, and the most */
  for (int j = 0; j < widest; j++) {
    bytes += (size_t)(plan.len[j] - max_len);
  }
  ContinueBuffers cb;
  cb.sb.d_first = NULL;
  cb.sb.h_len = ramd_zalloc((size_t)widest * sizeof(int));
  cb.sb.h_done = ramd_zalloc((size_t)widest * sizeof(int));
  cb.sb.h_rng = ramd_zalloc((size_t)widest * sizeof(rand_ctx));
  cb.sb.h_text = ramd_zalloc((size_t)widest * max_len);
  cb.h_prompt = ramd_zalloc(bytes);
  cb.h_off = ramd_zalloc((size_t)widest * sizeof(unsigned long long));
  cb.h_plen = ramd_zalloc((size_t)widest * sizeof(int));
  cb.h_state = cs->h_in || cs->h_out ? ramd_zalloc((size_t)widest * e->sh.H * sizeof(float)) : NULL;
  cb.sb.d_len = ramd_dev_alloc((size_t)widest * sizeof(int));
  cb.sb.d_done = ramd_dev_alloc((size_t)widest * sizeof(int));
  cb.sb.d_rng = ramd_dev_alloc((size_t)widest * sizeof(rand_ctx));
  cb.sb.d_text = ramd_dev_alloc((size_t)widest * max_len);
  cb.d_prompt = ramd_dev_alloc(bytes);
  cb.d_off = ramd_dev_alloc((size_t)widest * sizeof(unsigned long long));
  cb.d_plen = ramd_dev_alloc((size_t)widest * sizeof(int));
  int failed = 0;
  for (int w = 0; w < plan.n_waves; w++) {
    failed += continue_wave(e, net, &plan, w, r0, prompts, cs, max_len, bias, stop_point, alen, head, &cb, out, out_lens);
  }
  ramd_dev_free(cb.sb.d_len);
  ramd_dev_free(cb.sb.d_done);
  ramd_dev_free(cb.sb.d_rng);
  ramd_dev_free(cb.sb.d_text);
  ramd_dev_free(cb.d_prompt);
  ramd_dev_free(cb.d_off);
  ramd_dev_free(cb.d_plen);
  free(cb.sb.h_len);
  free(cb.sb.h_done);
  free(cb.sb.h_rng);
  free(cb.sb.h_text);
  free(cb.h_prompt);
  free(cb.h_off);
  free(cb.h_plen);
  free(cb.h_state);
  texts_plan_free(&plan);
  if (failed) {
    fprintf(stderr, "librecur_amd: %s: %d of %d texts met the attempt cap of the draw (an output row without a total)\n",
            who, failed, n_texts);
    return -1;
  }
  return 0;
}

int rnn_amd_continue_texts_from(RecurNN *net, const u8 *const *prompts, const int *prompt_lens, const u64 *seeds,
                                const rand_ctx *rng_in, int n_texts, int max_len, float bias, int stop_point,
                                int alphabet_len, int head, const float *h_in, float *h_out, u8 *out, int *out_lens,
                                rand_ctx *rng_out) {
  const ContinueStates cs = {.h_in = h_in, .h_out = h_out, .seeds = seeds, .rng_in = rng_in, .rng_out = rng_out};
  return continue_texts("rnn_amd_continue_texts_from", net, prompts, prompt_lens, n_texts, max_len, bias, stop_point,
                        alphabet_len, head, &cs, out, out_lens);
}

int rnn_amd_continue_texts(RecurNN *net, const u8 *const *prompts, const int *prompt_lens, const u64 *seeds, int n_texts,
                           int max_len, float bias, int stop_point, int alphabet_len, int head, u8 *out, int *out_lens,
                           rand_ctx *rng_out) {
  const ContinueStates cs = {.seeds = seeds, .rng_out = rng_out};
  return continue_texts("rnn_amd_continue_texts", net, prompts, prompt_lens, n_texts, max_len, bias, stop_point, alphabet_len,
                        head, &cs, out, out_lens);
}

/* rnn_char_confabulate's room rule (char_sampling.c): byte_len - (utf8 ? 5 : 1) bytes for symbols -- one may need four,
 * then the NUL.  Returns the room, or 0 after saying so and emptying every text */
static int room_for_texts(const RnnCharAlphabet *a, int n_texts, char **dest, int byte_len, int *bytes) {
  const int room = byte_len - ((a->flags & RNN_CHAR_FLAG_UTF8) ? 5 : 1);
  if (room > 0) {
    return room;
  }
  fprintf(stderr, "insufficient space to confabulate (%d bytes)\n", byte_len);
  for (int k = 0; k < n_texts; k++) {
    if (byte_len > 0) {
      dest[k][0] = 0;
    }
    bytes[k] = 0;
  }
  return 0;
}

/* the symbols-to-text loop of both character calls: text k's lens[k] symbols at syms + k * stride into dest[k], until the
 * room is used up */
static void symbols_to_texts(const RnnCharAlphabet *a, const u8 *syms, int stride, const int *lens, int n_texts, int room,
                             char **dest, int *bytes) {
  const int utf8 = (a->flags & RNN_CHAR_FLAG_UTF8) != 0;
  for (int k = 0; k < n_texts; k++) {
    int used = 0;
    for (int i = 0; i < lens[k] && used < room; i++) {
      used += ramd_put_codepoint(a->points[syms[(size_t)k * stride + i]], dest[k] + used, utf8);
    }
    dest[k][used] = 0;
    bytes[k] = used;
  }
}

/* rnn_char_confabulate's passage (char_sampling.c) n_texts times over, side by side: the same symbols-to-text loop under
 * the same room rule, on the symbols of one rnn_amd_sample_texts call */
int rnn_amd_char_confabulate_texts(RecurNN *net, RnnCharAlphabet *a, const u64 *seeds, int n_texts, int char_len, float bias,
                                   int prev_char, int stop_point, char **dest, int byte_len, int *bytes) {
  const char *who = "rnn_amd_char_confabulate_texts";
  if (!net || !a || n_texts < 0 || char_len < 0 || (n_texts > 0 && (!seeds || !dest || !bytes))) {
    fprintf(stderr, "librecur_amd: %s: %d texts of %d characters, or a NULL argument\n", who, n_texts, char_len);
    return -1;
  }
  const int room = room_for_texts(a, n_texts, dest, byte_len, bytes);
  if (room <= 0 || n_texts == 0) {
    return 0;
  }
  int *first = malloc((size_t)n_texts * sizeof(int));
  int *lens = calloc((size_t)n_texts, sizeof(int)); /* (a refused call writes none) */
  u8 *syms = malloc((size_t)n_texts * RAMD_MAX(char_len, 1));
  for (int k = 0; k < n_texts; k++) {
    first[k] = prev_char;
  }
  const int r = rnn_amd_sample_texts(net, first, seeds, n_texts, char_len, bias, stop_point, 0, 0, syms, lens, NULL);
  symbols_to_texts(a, syms, char_len, lens, n_texts, room, dest, bytes);
  free(first);
  free(lens);
  free(syms);
  return r;
}

/* the same with a prompt per passage: every prompt encoded as the alphabet says, one rnn_amd_continue_texts call, the
 * continuations turned into text under the same room rule */
int rnn_amd_char_continue_texts(RecurNN *net, RnnCharAlphabet *a, const char *const *prompts, const int *prompt_bytes,
                                const u64 *seeds, int n_texts, int char_len, float bias, int stop_point, char **dest,
                                int byte_len, int *bytes) {
  const char *who = "rnn_amd_char_continue_texts";
  if (!net || !a || n_texts < 0 || char_len < 0 || (n_texts > 0 && (!prompts || !prompt_bytes || !seeds || !dest || !bytes))) {
    fprintf(stderr, "librecur_amd: %s: %d texts of %d characters, or a NULL argument\n", who, n_texts, char_len);
    return -1;
  }
  if (n_texts == 0) {
    return 0;
  }
  u8 **enc = calloc((size_t)n_texts, sizeof(u8 *));
  int *plens = calloc((size_t)n_texts, sizeof(int));
  int *lens = calloc((size_t)n_texts, sizeof(int)); /* (a refused call writes none) */
  u8 *syms = malloc((size_t)n_texts * RAMD_MAX(char_len, 1));
  int r = 0;
  for (int k = 0; k < n_texts && r == 0; k++) {
    if (prompts[k] && prompt_bytes[k] >= 0) {
      enc[k] = rnn_char_alloc_encoded_text(a, prompts[k], prompt_bytes[k], &plens[k], NULL, false);
    }
    if (plens[k] < 1) {
      fprintf(stderr, "librecur_amd: %s: prompt %d encodes to no symbol\n", who, k);
      r = -1;
    }
  }
  if (r) { /* refused: nothing computed, every text empty */
    for (int k = 0; k < n_texts; k++) {
      if (byte_len > 0) {
        dest[k][0] = 0;
      }
      bytes[k] = 0;
    }
  } else {
    const int room = room_for_texts(a, n_texts, dest, byte_len, bytes);
    if (room > 0) {
      r = rnn_amd_continue_texts(net, (const u8 *const *)enc, plens, seeds, n_texts, char_len, bias, stop_point, 0, 0, syms,
                                 lens, NULL);
      symbols_to_texts(a, syms, char_len, lens, n_texts, room, dest, bytes);
    }
  }
  for (int k = 0; k < n_texts; k++) {
    free(enc[k]);
  }
  free(enc);
  free(plens);
  free(lens);
  free(syms);
  return r;
}

/* Prompts scored AND continued, every prompt fed once: one rnn_amd_run_texts_from hands back each prompt's sum and the
 * state behind its last symbol but one; the states, `repeats` times each, are where one rnn_amd_continue_texts_from goes
 * on from the prompts' last symbols */
int rnn_amd_char_score_and_continue_texts(RecurNN *net, RnnCharAlphabet *a, const char *const *prompts,
                                          const int *prompt_bytes, const u64 *seeds, int n_texts, int repeats, int char_len,
                                          float bias, int stop_point, char **dest, int byte_len, int *bytes,
                                          double *entropy) {
  const char *who = "rnn_amd_char_score_and_continue_texts";
  if (!net || !a || n_texts < 0 || char_len < 0 || repeats < 1 || (n_texts > 0 && repeats > INT_MAX / n_texts) ||
      (n_texts > 0 && (!prompts || !prompt_bytes || !seeds || !dest || !bytes || !entropy))) {
    fprintf(stderr, "librecur_amd: %s: %d texts %d times of %d characters, or a NULL argument\n", who, n_texts, repeats,
            char_len);
    return -1;
  }
  if (n_texts == 0) {
    return 0;
  }
  const int rows = n_texts * repeats;
  const size_t H = (size_t)net->h_size;
  u8 **enc = calloc((size_t)n_texts, sizeof(u8 *));
  int *plens = calloc((size_t)n_texts, sizeof(int));
  int *lens = calloc((size_t)rows, sizeof(int)); /* (a refused call writes none) */
  u8 *syms = malloc((size_t)rows * RAMD_MAX(char_len, 1));
  int r = 0;
  for (int k = 0; k < n_texts && r == 0; k++) {
    if (prompts[k] && prompt_bytes[k] >= 0) {
      enc[k] = rnn_char_alloc_encoded_text(a, prompts[k], prompt_bytes[k], &plens[k], NULL, false);
    }
    if (plens[k] < 1) {
      fprintf(stderr, "librecur_amd: %s: prompt %d encodes to no symbol\n", who, k);
      r = -1;
    }
  }
  const int room = r ? 0 : room_for_texts(a, rows, dest, byte_len, bytes);
  if (r) { /* refused: nothing computed, every text empty */
    for (int i = 0; i < rows; i++) {
      if (byte_len > 0) {
        dest[i][0] = 0;
      }
      bytes[i] = 0;
    }
  } else if (room > 0) {
    float *state = malloc((size_t)n_texts * H * sizeof(float));
    float *start = malloc((size_t)rows * H * sizeof(float));
    u8 *last = malloc((size_t)rows);
    const u8 **last_of = malloc((size_t)rows * sizeof(u8 *));
    int *ones = malloc((size_t)rows * sizeof(int));
    r = rnn_amd_run_texts_from(net, (const u8 *const *)enc, plens, NULL, n_texts, 0, NULL, state, entropy);
    for (int k = 0; r == 0 && k < n_texts; k++) {
      entropy[k] = entropy[k] / -(double)(plens[k] - 1); /* rnn_amd_char_cross_entropy_texts's expression, ignore_first 0 */
      for (int i = k * repeats; i < (k + 1) * repeats; i++) {
        memcpy(start + (size_t)i * H, state + (size_t)k * H, H * sizeof(float));
        last[i] = enc[k][plens[k] - 1];
        last_of[i] = last + i;
        ones[i] = 1;
      }
    }
    if (r == 0) {
      r = rnn_amd_continue_texts_from(net, last_of, ones, seeds, NULL, rows, char_len, bias, stop_point, 0, 0, start, NULL,
                                      syms, lens, NULL);
    }
    symbols_to_texts(a, syms, char_len, lens, rows, room, dest, bytes);
    free(state);
    free(start);
    free(last);
    free(last_of);
    free(ones);
  }
  for (int k = 0; k < n_texts; k++) {
    free(enc[k]);
  }
  free(enc);
  free(plens);
  free(lens);
  free(syms);
  return r;
}
