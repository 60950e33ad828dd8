/* texts_api.c -- many texts against one net in one batched device run (gnu11 C): rnn_amd_run_texts and
 * rnn_amd_run_texts_heads, the set form of rnn_amd_run_text / _heads (net_api.c), and rnn_amd_trace_texts, which hands
 * back per symbol what those add up (k_texts_step's trace form).  Where those feed one net a symbol per
 * launch sequence, these give every text a forward-only state row of the engine's own (opened, and the call's staging
 * buffers owned, by rows_host.c, which the other batched calls share) and run the rows together: which
 * text gets which row, in how many waves and with how many rows at each step is texts_plan.h's business; between two
 * forward passes of the rows there is one launch (k_texts_step, kernels_rows.hip) that scores the step just computed and
 * builds the input rows of the next.  The net the caller passes is read -- its weights, its hidden row -- and not written.
 * The public calls are the _from forms (rnn_amd_run_texts_from, rnn_amd_trace_texts_from): every text's start state from
 * the caller's h_in and its final state into the caller's h_out, either of them NULL for "the net's hidden row" and "not
 * wanted"; which state belongs to which row is texts_states.h's business.  The forms without states call them with NULLs. */
#define RAMD_HIP_HOST 1
#include <limits.h>
#include "rnn_host.h"
#include "texts_plan.h"
#include "texts_states.h"

int ramd_run_texts_refused(const char *who, const RecurNN *net, const u8 *const *texts, const int *lens, int n_texts,
                           int alphabet_len, const void *out) {
  if (!net || n_texts < 0) {
    fprintf(stderr, "librecur_amd: %s: %d texts\n", who, n_texts);
    return -1;
  }
  if (ramd_texts_net_refused(who, net, alphabet_len)) {
    return -1;
  }
  if (n_texts > 0 && (!texts || !lens || !out)) {
    fprintf(stderr, "librecur_amd: %s: a NULL array for %d texts\n", who, n_texts);
    return -1;
  }
  for (int k = 0; k < n_texts; k++) {
    if (lens[k] >= 2 && !texts[k]) {
      fprintf(stderr, "librecur_amd: %s: text %d is NULL\n", who, k);
      return -1;
    }
  }
  return 0;
}

/* what a call wants back: the sums form (one double per text and head in sums; NULL: the texts are fed and nothing is
 * scored, rnn_char_prime's loop), or the trace form (every float the sums form would add, in logp, and -- unless NULL --
 * the best guess next to each); and the states: every text's start state in h_in (NULL: the net's hidden row), its final
 * state into h_out (NULL: not wanted) */
typedef struct TextsWanted {
  int trace;
  double *sums;
  float *const *logp;
  u8 *const *guess;
  const float *h_in;
  float *h_out;
} TextsWanted;

/* one wave of the plan on the state rows from r0 on; the d_* arrays have room for the plan's first (largest) wave, the
 * h_* ones are the pinned-or-not host sides of them and stay untouched until the wave's synchronisation.  The sums form
 * uses skip and acc; the trace form off_tr and trace: a wave's floats, then -- with guesses -- its bytes, in ONE buffer
 * so that one copy brings both back, row j's entries from off_tr[j] on in either */
typedef struct TextsBuffers {
  u8 *h_text, *d_text;
  unsigned long long *h_off, *d_off;
  int *d_skip;
  double *h_acc, *d_acc;
  unsigned long long *h_off_tr, *d_off_tr;
  u8 *h_trace, *d_trace;
  float *h_state; /* [rows][H] the wave's states on their way in and out, or NULL */
} TextsBuffers;

static void run_wave(const RamdRows *rows, const TextsPlan *plan, int w, const u8 *const *texts, int alphabet_len,
                     int n_sums, const TextsBuffers *tb, const TextsWanted *want) {
  RamdEngine *e = rows->e;
  const RamdShape *s = &e->sh;
  const TextsWave *wave = &plan->waves[w];
  const int n = wave->nrows;
  const int alen = alphabet_len ? alphabet_len : s->output_size;
  size_t at = 0;
  for (int j = 0; j < n; j++) {
    const int len = plan->len[wave->row0 + j];
    tb->h_off[j] = at;
    memcpy(tb->h_text + at, texts[plan->order[wave->row0 + j]], (size_t)len);
    at += (size_t)len;
  }
  ramd_h2d(tb->d_text, tb->h_text, at);
  ramd_h2d(tb->d_off, tb->h_off, (size_t)n * sizeof(unsigned long long));
  size_t traced = 0; /* the wave's traced values */
  u8 *d_guess = NULL;
  if (!want->trace) {
    ramd_h2d(tb->d_skip, plan->skip + wave->row0, (size_t)n * sizeof(int));
    HIP_OK(hipMemsetAsync(tb->d_acc, 0, (size_t)n * n_sums * sizeof(double), ramd_stream));
  } else {
    traced = texts_plan_trace_offsets(plan, w, n_sums, tb->h_off_tr);
    ramd_h2d(tb->d_off_tr, tb->h_off_tr, (size_t)n * sizeof(unsigned long long));
    d_guess = want->guess ? tb->d_trace + traced * sizeof(float) : NULL;
  }
  /* (the sums form leaves trace NULL, and the launcher takes its form from that) */
  RamdTextsStep step = {.text = tb->d_text, .off = tb->d_off, .skip = tb->d_skip, .acc = tb->d_acc, .off_tr = tb->d_off_tr,
                        .trace = want->trace ? (float *)tb->d_trace : NULL, .guess = d_guess, .row0 = rows->r0, .alen = alen,
                        .n_sums = n_sums};
  step.hid0 = ramd_rows_states_in(rows, plan, w, want->h_in, tb->h_state);
  for (int t = 0; t <= wave->steps; t++) {
    step.t_score = t - 1;
    step.a_score = step.a_feed; /* a(t - 1): the rows whose step t - 1 waits to be scored */
    step.t_feed = t;
    step.a_feed = t < wave->steps ? texts_plan_active(plan, w, t) : 0;
    ramd_launch_texts_step(ramd_stream, s, &e->b, &step);
    step.hid0 = NULL;
    if (step.a_feed) {
      ramd_rows_forward(rows, step.a_feed);
    }
  }
  if (want->sums) {
    ramd_d2h(tb->h_acc, tb->d_acc, (size_t)n * n_sums * sizeof(double));
  } else if (want->trace) {
    ramd_d2h(tb->h_trace, tb->d_trace, traced * (sizeof(float) + (want->guess ? 1 : 0)));
  }
  /* (a row's last forward pass was its last writer: the passes after it had fewer rows) */
  ramd_rows_states_out(rows, n, want->h_out ? tb->h_state : NULL);
  ramd_dsync(); /* the wave's one synchronisation */
  if (want->h_out) {
    texts_states_unpack(plan, w, tb->h_state, s->H, want->h_out);
  }
  for (int j = 0; j < n && (want->sums || want->trace); j++) {
    const int k = plan->order[wave->row0 + j];
    if (want->sums) {
      memcpy(want->sums + (size_t)k * n_sums, tb->h_acc + (size_t)j * n_sums, (size_t)n_sums * sizeof(double));
      continue;
    }
    const size_t count = (size_t)(plan->len[wave->row0 + j] - 1) * n_sums;
    memcpy(want->logp[k], tb->h_trace + tb->h_off_tr[j] * sizeof(float), count * sizeof(float));
    if (want->guess) {
      memcpy(want->guess[k], tb->h_trace + traced * sizeof(float) + tb->h_off_tr[j], count);
    }
  }
}

static int run_texts(const char *who, RecurNN *net, const u8 *const *texts, const int *lens, const int *skips, int n_texts,
                     int alphabet_len, const TextsWanted *want) {
  double *sums = want->sums;
  float *const *logp = want->logp;
  u8 *const *guess = want->guess;
  /* (the sums form may leave out its sums where it hands back states: the texts are fed and nothing is scored) */
  const void *result = want->trace ? (const void *)logp : sums ? (const void *)sums : (const void *)want->h_out;
  if (ramd_run_texts_refused(who, net, texts, lens, n_texts, alphabet_len, result)) {
    return -1;
  }
  const int n_sums = alphabet_len ? net->output_size / alphabet_len : 1;
  if (!want->trace) {
    for (size_t q = 0; sums && q < (size_t)n_texts * n_sums; q++) {
      sums[q] = 0.0;
    }
  } else {
    if (guess && (alphabet_len ? alphabet_len : net->output_size) > 256) {
      fprintf(stderr, "librecur_amd: %s: a guess among %d outputs does not fit a byte\n", who,
              alphabet_len ? alphabet_len : net->output_size);
      return -1;
    }
    for (int k = 0; k < n_texts; k++) {
      if (lens[k] >= 2 && (!logp[k] || (guess && !guess[k]))) {
        fprintf(stderr, "librecur_amd: %s: text %d has no array to be traced into\n", who, k);
        return -1;
      }
    }
  }
  TextsPlan plan;
  if (texts_plan_make(&plan, lens, skips, n_texts, TEXTS_PLAN_WIDTH)) {
    fprintf(stderr, "librecur_amd: %s: out of memory planning %d texts\n", who, n_texts);
    return -1;
  }
  if (ramd_texts_fill_rowless(net, lens, n_texts, plan.n_rows, want->h_in, want->h_out)) {
    fprintf(stderr, "librecur_amd: %s: out of memory\n", who);
    texts_plan_free(&plan);
    return -1;
  }
  if (plan.n_rows == 0) { /* nothing to score: no device is asked for */
    return 0;
  }
  if (!want->trace && !sums) {
    for (int r = 0; r < plan.n_rows; r++) {
      plan.skip[r] = INT_MAX; /* fed, never scored */
    }
  }
  const int widest = plan.waves[0].nrows;
  RamdRows rows;
  ramd_rows_open(&rows, net, widest);
  size_t bytes = 0;
  for (int j = 0; j < widest; j++) {
    bytes += (size_t)plan.len[j];
  }
  TextsBuffers tb = {0};
  tb.h_text = ramd_rows_host(&rows, bytes);
  tb.h_off = ramd_rows_host(&rows, (size_t)widest * sizeof(unsigned long long));
  tb.d_text = ramd_rows_dev(&rows, bytes);
  tb.d_off = ramd_rows_dev(&rows, (size_t)widest * sizeof(unsigned long long));
  if (want->h_in || want->h_out) {
    tb.h_state = ramd_rows_host(&rows, (size_t)widest * rows.e->sh.H * sizeof(float));
  }
  if (!want->trace) {
    tb.h_acc = ramd_rows_host(&rows, (size_t)widest * n_sums * sizeof(double));
    tb.d_skip = ramd_rows_dev(&rows, (size_t)widest * sizeof(int));
    tb.d_acc = ramd_rows_dev(&rows, (size_t)widest * n_sums * sizeof(double));
  } else { /* the first wave has the most rows and the longest texts: the largest trace */
    tb.h_off_tr = ramd_rows_host(&rows, (size_t)widest * sizeof(unsigned long long));
    const size_t room = texts_plan_trace_offsets(&plan, 0, n_sums, tb.h_off_tr) * (sizeof(float) + (guess ? 1 : 0));
    tb.h_trace = ramd_rows_host(&rows, room);
    tb.d_off_tr = ramd_rows_dev(&rows, (size_t)widest * sizeof(unsigned long long));
    tb.d_trace = ramd_rows_dev(&rows, room);
  }
  for (int w = 0; w < plan.n_waves; w++) {
    run_wave(&rows, &plan, w, texts, alphabet_len, n_sums, &tb, want);
  }
  ramd_rows_close(&rows);
  texts_plan_free(&plan);
  return 0;
}

int rnn_amd_run_texts_from(RecurNN *net, const u8 *const *texts, const int *lens, const int *skips, int n_texts,
                           int alphabet_len, const float *h_in, float *h_out, double *sums) {
  const TextsWanted want = {.sums = sums, .h_in = h_in, .h_out = h_out};
  return run_texts("rnn_amd_run_texts_from", net, texts, lens, skips, n_texts, alphabet_len, &want);
}

int rnn_amd_run_texts(RecurNN *net, const u8 *const *texts, const int *lens, const int *skips, int n_texts,
                      double *sums) {
  const TextsWanted want = {.sums = sums};
  return run_texts("rnn_amd_run_texts", net, texts, lens, skips, n_texts, 0, &want);
}

int rnn_amd_run_texts_heads(RecurNN *net, const u8 *const *texts, const int *lens, const int *skips, int n_texts,
                            int alphabet_len, double *sums) {
  if (alphabet_len < 1) {
    fprintf(stderr, "librecur_amd: rnn_amd_run_texts_heads: heads of %d outputs\n", alphabet_len);
    return -1;
  }
  const TextsWanted want = {.sums = sums};
  return run_texts("rnn_amd_run_texts_heads", net, texts, lens, skips, n_texts, alphabet_len, &want);
}

int rnn_amd_trace_texts_from(RecurNN *net, const u8 *const *texts, const int *lens, int n_texts, int alphabet_len,
                             const float *h_in, float *h_out, float *const *logp, u8 *const *guess) {
  const TextsWanted want = {.trace = 1, .logp = logp, .guess = guess, .h_in = h_in, .h_out = h_out};
  return run_texts("rnn_amd_trace_texts_from", net, texts, lens, NULL, n_texts, alphabet_len, &want);
}

int rnn_amd_trace_texts(RecurNN *net, const u8 *const *texts, const int *lens, int n_texts, int alphabet_len,
                        float *const *logp, u8 *const *guess) {
  const TextsWanted want = {.trace = 1, .logp = logp, .guess = guess};
  return run_texts("rnn_amd_trace_texts", net, texts, lens, NULL, n_texts, alphabet_len, &want);
}
