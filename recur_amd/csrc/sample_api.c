/* sample_api.c -- many texts drawn from one net in one batched device run (gnu11 C): rnn_amd_continue_texts, the
 * generative counterpart of rnn_amd_run_texts (texts_api.c), rnn_amd_sample_texts, which is that call with every prompt
 * one symbol, and their character layers.  Where rnn_char_confabulate (char_sampling.c) visits the host for every symbol
 * of one net -- the output row comes back, the host draws, the generator goes out again -- these give every text a
 * forward-only state row of the engine's own (rows_host.c) and a generator of its own in a buffer of the call's, and run
 * the rows together.  The rows are laid out by prompt length + max_len (texts_plan.h, as rnn_amd_run_texts lays out its
 * texts), and between two forward passes of the rows there is one launch (k_texts_continue, kernels_rows.hip) that feeds
 * a row its prompt or draws its next symbol on the device (sample_rule.h) and builds the input row of the next pass from
 * it, as continue_rule.h says.  There is ONE wave loop, continue_wave, and one body behind the refusals, draw_texts:
 * the sampler hands it its first symbols as ints (they may lie above 255, so they do not travel as prompt bytes) and
 * equal lengths, for which the plan keeps the caller's order in waves of 256.  The net the caller passes is read -- its
 * weights, its hidden row -- and not written.
 * rnn_amd_continue_texts_from is the call with every row's start state and generator from the caller's arrays and its
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

/* the device and host sides of one wave's arrays, with room for the plan's first (largest) wave; the prompts' three, or
 * d_first alone where every row's prompt is the one symbol first[k] */
typedef struct ContinueBuffers {
  int *d_len, *d_done, *h_len, *h_done;
  rand_ctx *d_rng, *h_rng;
  u8 *d_text, *h_text;
  u8 *h_prompt, *d_prompt;
  unsigned long long *h_off, *d_off;
  int *h_plen, *d_plen;
  int *d_first;
  float *h_state; /* [rows][H] the wave's states on their way in and out, or NULL */
} ContinueBuffers;

/* what a call's rows start from -- their prompts, or (first != NULL) one symbol each, which may lie above 255 -- and
 * where, and what it hands back of them besides the text: start states and generators (NULL: the net's hidden row,
 * init_rand64 of the seeds), final states and generators (NULL: not wanted) */
typedef struct ContinueCall {
  const u8 *const *prompts;
  const int *first;
  const float *h_in;
  float *h_out;
  const u64 *seeds;
  const rand_ctx *rng_in;
  rand_ctx *rng_out;
} ContinueCall;

/* row k's generator before its first draw */
static rand_ctx start_generator(const ContinueCall *cc, int k) {
  rand_ctx g;
  if (cc->rng_in) {
    g = cc->rng_in[k];
  } else {
    ramd_init_rand64(&g, cc->seeds[k]);
  }
  return g;
}

/* wave w of the plan (its len is prompt length + max_len) on the call's state rows; returns the number of rows whose
 * draw failed */
static int continue_wave(const RamdRows *rows, const TextsPlan *plan, int w, const ContinueCall *cc, int max_len,
                         float bias, int stop_point, int alen, int head, const ContinueBuffers *cb, u8 *out,
                         int *out_lens) {
  RamdEngine *e = rows->e;
  const RamdShape *s = &e->sh;
  const TextsWave *wave = &plan->waves[w];
  const int n = wave->nrows;
  size_t at = 0;
  for (int j = 0; j < n; j++) {
    const int k = plan->order[wave->row0 + j], plen = plan->len[wave->row0 + j] - max_len;
    if (!cc->first) {
      cb->h_off[j] = at;
      cb->h_plen[j] = plen;
      memcpy(cb->h_prompt + at, cc->prompts[k], (size_t)plen);
      at += (size_t)plen;
    }
    cb->h_rng[j] = start_generator(cc, k);
  }
  if (cc->first) { /* (equal lengths: the plan keeps the caller's order, row row0 + j is text row0 + j) */
    ramd_h2d(cb->d_first, cc->first + wave->row0, (size_t)n * sizeof(int));
  } else {
    ramd_h2d(cb->d_prompt, cb->h_prompt, at);
    ramd_h2d(cb->d_off, cb->h_off, (size_t)n * sizeof(unsigned long long));
    ramd_h2d(cb->d_plen, cb->h_plen, (size_t)n * sizeof(int));
  }
  ramd_h2d(cb->d_rng, cb->h_rng, (size_t)n * sizeof(rand_ctx));
  HIP_OK(hipMemsetAsync(cb->d_len, 0, (size_t)n * sizeof(int), ramd_stream));
  HIP_OK(hipMemsetAsync(cb->d_done, 0, (size_t)n * sizeof(int), ramd_stream));
  /* (hid0 stays: the kernel takes it at t == 0 alone, continue_rule.h's on_hid0; rows: the rows launch t is for, those
   * that were fed after launch t - 1) */
  RamdTextsContinue step = {.prompt = cb->d_prompt, .off = cb->d_off, .plen = cb->d_plen, .first = cb->d_first,
                            .rng = cb->d_rng, .text = cb->d_text, .len = cb->d_len, .done = cb->d_done, .row0 = rows->r0,
                            .rows = n, .alen = alen, .head = head, .max_len = max_len, .stop_point = stop_point, .bias = bias};
  step.hid0 = ramd_rows_states_in(rows, plan, w, cc->h_in, cb->h_state);
  const int lead = plan->len[wave->row0] - max_len; /* the wave's longest row: its launches are the wave's */
  for (int t = 0;; t++) {
    const ContinueStep st = continue_step(lead, max_len, t);
    if (st.what == CONTINUE_IDLE) {
      break;
    }
    step.t = t;
    ramd_launch_texts_continue(ramd_stream, s, &e->b, &step);
    if (!st.feeds) { /* the longest row's last draw */
      break;
    }
    const int a = texts_plan_active(plan, w, t); /* the rows that are fed after launch t: a prefix (texts_plan.h) */
    if (t > 0 && t % SAMPLE_CHECK_EVERY == 0) { /* has every such row met its stop symbol?  then the rest would run on nothing */
      ramd_d2h(cb->h_done, cb->d_done, (size_t)a * sizeof(int));
      ramd_dsync();
      int running = 0;
      for (int j = 0; j < a; j++) {
        running += cb->h_done[j] == 0;
      }
      if (!running) {
        break;
      }
    }
    ramd_rows_forward(rows, a);
    step.rows = a;
  }
  ramd_d2h(cb->h_text, cb->d_text, (size_t)n * max_len);
  ramd_d2h(cb->h_len, cb->d_len, (size_t)n * sizeof(int));
  ramd_d2h(cb->h_done, cb->d_done, (size_t)n * sizeof(int));
  ramd_d2h(cb->h_rng, cb->d_rng, (size_t)n * sizeof(rand_ctx));
  /* every row has had a forward pass (launch 0 feeds them all), and its hidden row is the one after its last feed: a
   * pass over a row that was not fed since recomputes that row from the same input row, and a look above ends the wave
   * only where its launch fed no row (every row it could have fed is done) */
  ramd_rows_states_out(rows, n, cc->h_out ? cb->h_state : NULL);
  ramd_dsync(); /* the wave's synchronisation */
  if (cc->h_out) {
    texts_states_unpack(plan, w, cb->h_state, s->H, cc->h_out);
  }
  int failed = 0;
  for (int j = 0; j < n; j++) {
    const int k = plan->order[wave->row0 + j];
    const int len = RAMD_MIN(RAMD_MAX(cb->h_len[j], 0), max_len);
    memcpy(out + (size_t)k * max_len, cb->h_text + (size_t)j * max_len, (size_t)len);
    out_lens[k] = len;
    failed += cb->h_done[j] == 2;
    if (cc->rng_out) {
      cc->rng_out[k] = cb->h_rng[j];
    }
  }
  return failed;
}

/* what every drawing call runs behind its refusals and its returns that ask for no device: n_texts >= 1 rows of
 * prompt_lens[k] (with cc->first: 1) + max_len >= 2 launches each, planned, opened and run wave by wave */
static int draw_texts(const char *who, RecurNN *net, const int *prompt_lens, int n_texts, int max_len, float bias,
                      int stop_point, int alphabet_len, int head, const ContinueCall *cc, u8 *out, int *out_lens) {
  int *lens = ramd_zalloc((size_t)n_texts * sizeof(int)); /* what a row is planned by: the forward passes it takes, plus 1 */
  TextsPlan plan;
  for (int k = 0; k < n_texts; k++) {
    lens[k] = (cc->first ? 1 : prompt_lens[k]) + max_len; /* at least 2: every prompt takes a row */
  }
  const int unplanned = texts_plan_make(&plan, lens, NULL, n_texts, TEXTS_PLAN_WIDTH);
  free(lens);
  if (unplanned) {
    fprintf(stderr, "librecur_amd: %s: out of memory planning %d texts\n", who, n_texts);
    return -1;
  }
  const int alen = alphabet_len ? alphabet_len : net->output_size;
  const int widest = plan.waves[0].nrows;
  RamdRows rows;
  ramd_rows_open(&rows, net, widest);
  size_t bytes = 0; /* of the first wave's prompts: the longest rows, and the most */
  for (int j = 0; j < widest; j++) {
    bytes += (size_t)(plan.len[j] - max_len);
  }
  ContinueBuffers cb = {0};
  cb.h_len = ramd_rows_host(&rows, (size_t)widest * sizeof(int));
  cb.h_done = ramd_rows_host(&rows, (size_t)widest * sizeof(int));
  cb.h_rng = ramd_rows_host(&rows, (size_t)widest * sizeof(rand_ctx));
  cb.h_text = ramd_rows_host(&rows, (size_t)widest * max_len);
  if (!cc->first) {
    cb.h_prompt = ramd_rows_host(&rows, bytes);
    cb.h_off = ramd_rows_host(&rows, (size_t)widest * sizeof(unsigned long long));
    cb.h_plen = ramd_rows_host(&rows, (size_t)widest * sizeof(int));
  }
  if (cc->h_in || cc->h_out) {
    cb.h_state = ramd_rows_host(&rows, (size_t)widest * rows.e->sh.H * sizeof(float));
  }
  if (cc->first) {
    cb.d_first = ramd_rows_dev(&rows, (size_t)widest * sizeof(int));
  }
  cb.d_len = ramd_rows_dev(&rows, (size_t)widest * sizeof(int));
  cb.d_done = ramd_rows_dev(&rows, (size_t)widest * sizeof(int));
  cb.d_rng = ramd_rows_dev(&rows, (size_t)widest * sizeof(rand_ctx));
  cb.d_text = ramd_rows_dev(&rows, (size_t)widest * max_len);
  if (!cc->first) {
    cb.d_prompt = ramd_rows_dev(&rows, bytes);
    cb.d_off = ramd_rows_dev(&rows, (size_t)widest * sizeof(unsigned long long));
    cb.d_plen = ramd_rows_dev(&rows, (size_t)widest * sizeof(int));
  }
  int failed = 0;
  for (int w = 0; w < plan.n_waves; w++) {
    failed += continue_wave(&rows, &plan, w, cc, max_len, bias, stop_point, alen, head, &cb, out, out_lens);
  }
  ramd_rows_close(&rows);
  texts_plan_free(&plan);
  if (failed) {
    fprintf(stderr, "librecur_amd: %s: %d of %d texts met the attempt cap of the draw (an output row without a total)\n",
            who, failed, n_texts);
    return -1;
  }
  return 0;
}

/* every row a one-symbol prompt, first[k], on the net's hidden row: continue_rule.h's schedule for plen == 1 is the
 * sampler's (launch 0 feeds the first symbol on hid0, launch t >= 1 draws index t - 1 and feeds the pick unless it was
 * the last), and a plan over equal lengths keeps the caller's order in waves of TEXTS_PLAN_WIDTH */
int rnn_amd_sample_texts(RecurNN *net, const int *first, const u64 *seeds, int n_texts, int max_len, float bias,
                         int stop_point, int alphabet_len, int head, u8 *out, int *out_lens, rand_ctx *rng_out) {
  const char *who = "rnn_amd_sample_texts";
  if (sample_texts_refused(who, net, first, seeds, n_texts, max_len, alphabet_len, head, out, out_lens)) {
    return -1;
  }
  if (n_texts == 0 || max_len == 0) {
    return nothing_to_draw(seeds, n_texts, out_lens, rng_out);
  }
  const ContinueCall cc = {.first = first, .seeds = seeds, .rng_out = rng_out};
  return draw_texts(who, net, NULL, n_texts, max_len, bias, stop_point, alphabet_len, head, &cc, out, out_lens);
}

static int continue_texts(const char *who, RecurNN *net, const int *prompt_lens, int n_texts, int max_len, float bias,
                          int stop_point, int alphabet_len, int head, const ContinueCall *cc, u8 *out, int *out_lens) {
  if (continue_texts_refused(who, net, cc->prompts, prompt_lens,
                             cc->rng_in ? (const void *)cc->rng_in : (const void *)cc->seeds, n_texts, max_len,
                             alphabet_len, head, out, out_lens)) {
    return -1;
  }
  if (n_texts == 0) {
    return 0;
  }
  if (max_len == 0) { /* nothing to draw: lengths zeroed, generators and states as they start, no device asked for... */
    for (int k = 0; k < n_texts; k++) {
      out_lens[k] = 0;
      if (cc->rng_out) {
        cc->rng_out[k] = start_generator(cc, k);
      }
    }
    /* (... unless the start state is the net's hidden row and only the device has it.  No text takes a row) */
    if (ramd_texts_fill_rowless(net, out_lens, n_texts, 0, cc->h_in, cc->h_out)) {
      fprintf(stderr, "librecur_amd: %s: out of memory\n", who);
      return -1;
    }
    return 0;
  }
  return draw_texts(who, net, prompt_lens, n_texts, max_len, bias, stop_point, alphabet_len, head, cc, out, out_lens);
}

int rnn_amd_continue_texts_from(RecurNN *net, const u8 *const *prompts, const int *prompt_lens, const u64 *seeds,
                                const rand_ctx *rng_in, int n_texts, int max_len, float bias, int stop_point,
                                int alphabet_len, int head, const float *h_in, float *h_out, u8 *out, int *out_lens,
                                rand_ctx *rng_out) {
  const ContinueCall cc = {.prompts = prompts, .h_in = h_in, .h_out = h_out, .seeds = seeds, .rng_in = rng_in,
                             .rng_out = rng_out};
  return continue_texts("rnn_amd_continue_texts_from", net, prompt_lens, n_texts, max_len, bias, stop_point, alphabet_len,
                        head, &cc, out, out_lens);
}

int rnn_amd_continue_texts(RecurNN *net, const u8 *const *prompts, const int *prompt_lens, const u64 *seeds, int n_texts,
                           int max_len, float bias, int stop_point, int alphabet_len, int head, u8 *out, int *out_lens,
                           rand_ctx *rng_out) {
  const ContinueCall cc = {.prompts = prompts, .seeds = seeds, .rng_out = rng_out};
  return continue_texts("rnn_amd_continue_texts", net, prompt_lens, n_texts, max_len, bias, stop_point, alphabet_len, head,
                        &cc, out, out_lens);
}

/* nothing computed: every text empty */
static void empty_texts(int n_texts, char **dest, int byte_len, int *bytes) {
  for (int k = 0; k < n_texts; k++) {
    if (byte_len > 0) {
      dest[k][0] = 0;
    }
    bytes[k] = 0;
  }
}

/* every prompt encoded as the alphabet says into enc[k] (the caller's to free, NULL where there is none) and plens[k];
 * returns -1 after saying so at the first prompt that encodes to no symbol */
static int encode_prompts(const char *who, RnnCharAlphabet *a, const char *const *prompts, const int *prompt_bytes,
                          int n_texts, u8 **enc, int *plens) {
  for (int k = 0; k < n_texts; k++) {
    if (prompts[k] && prompt_bytes[k] >= 0) {
      enc[k] = rnn_char_alloc_encoded_text(a, prompts[k], prompt_bytes[k], &plens[k], NULL, false);
    }
    if (plens[k] < 1) {
      fprintf(stderr, "librecur_amd: %s: prompt %d encodes to no symbol\n", who, k);
      return -1;
    }
  }
  return 0;
}

/* rnn_char_confabulate's room rule (char_sampling.c): byte_len - (utf8 ? 5 : 1) bytes for symbols -- one may need four,
 * then the NUL.  Returns the room, or 0 after saying so and emptying every text */
static int room_for_texts(const RnnCharAlphabet *a, int n_texts, char **dest, int byte_len, int *bytes) {
  const int room = byte_len - ((a->flags & RNN_CHAR_FLAG_UTF8) ? 5 : 1);
  if (room > 0) {
    return room;
  }
  fprintf(stderr, "insufficient space to confabulate (%d bytes)\n", byte_len);
  empty_texts(n_texts, dest, byte_len, bytes);
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
  int r = encode_prompts(who, a, prompts, prompt_bytes, n_texts, enc, plens);
  if (r) { /* refused */
    empty_texts(n_texts, dest, byte_len, bytes);
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
  int r = encode_prompts(who, a, prompts, prompt_bytes, n_texts, enc, plens);
  const int room = r ? 0 : room_for_texts(a, rows, dest, byte_len, bytes);
  if (r) { /* refused */
    empty_texts(rows, dest, byte_len, bytes);
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
