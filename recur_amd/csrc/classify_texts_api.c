/* classify_texts_api.c -- many texts against one classifier net in one batched device run (gnu11 C):
 * rnn_amd_classify_texts, the batched form of text-classify-results.c:83-122 (one_hot_opinion of every symbol, the host's
 * softmax over the class outputs, sum[k] += a, sumsq[k] += a * a) and of the validation block of rnn_char_classify_epoch
 * (charmodel-classify.c:174-196: the same loop held against every symbol's class).  It is texts_api.c with every symbol
 * fed AND scored, as seqs_api.c's frames are: every text gets a forward-only state row of the engine's own (rows_host.c),
 * texts_plan.h orders the rows and cuts the waves -- it is handed a text of len + 1 symbols for one of len, which has that
 * text's len forward passes --, between two forward passes of the rows there is one launch (k_classify_step,
 * kernels_rows.hip) that adds the softmax of the outputs just computed to the rows' accumulators and builds the input rows
 * of the next pass, and the states travel as texts_states.h says.  Texts and class bytes go up whole, a byte per symbol;
 * per wave there is one synchronisation, behind which the accumulators come back.  Which symbol is fed, scored or counted
 * is classify_rule.h's business.  The net the caller passes is read -- its weights, its hidden row -- and not written. */
#define RAMD_HIP_HOST 1
#include <limits.h>
#include "rnn_host.h"
#include "classify_rule.h"
#include "texts_plan.h"
#include "texts_states.h"

#define WHO "rnn_amd_classify_texts"

/* the refusals, which need no device: -1 with a line on stderr, else 0 */
static int classify_refused(const RecurNN *net, const u8 *const *texts, const int *lens, const u8 *const *classes,
                            int n_texts, const double *sums) {
  if (!net || n_texts < 0) {
    fprintf(stderr, "librecur_amd: " WHO ": %d texts\n", n_texts);
    return -1;
  }
  if (ramd_texts_net_refused(WHO, net, 0)) {
    return -1;
  }
  if (n_texts > 0 && (!texts || !lens || !sums)) {
    fprintf(stderr, "librecur_amd: " WHO ": a NULL array for %d texts\n", n_texts);
    return -1;
  }
  for (int k = 0; k < n_texts; k++) {
    if (lens[k] < 0 || lens[k] == INT_MAX) {
      fprintf(stderr, "librecur_amd: " WHO ": text %d has %d symbols\n", k, lens[k]);
      return -1;
    }
    if (lens[k] >= 1 && !texts[k]) {
      fprintf(stderr, "librecur_amd: " WHO ": text %d is NULL\n", k);
      return -1;
    }
    for (int j = 0; j < lens[k]; j++) {
      if (texts[k][j] >= net->input_size) {
        fprintf(stderr, "librecur_amd: " WHO ": text %d has symbol %d at %d, the net has %d inputs\n", k, texts[k][j], j,
                net->input_size);
        return -1;
      }
      if (classes && classes[k] && !classify_class_ok(classes[k][j], net->output_size)) {
        fprintf(stderr, "librecur_amd: " WHO ": text %d has class %d at %d, the net has %d outputs\n", k, classes[k][j], j,
                net->output_size);
        return -1;
      }
    }
  }
  return 0;
}

/* what a call wants back */
typedef struct ClassifyWanted {
  const u8 *const *texts;
  const u8 *const *classes; /* or NULL */
  const float *h_in;
  float *h_out;
  double *sums, *sumsqs;
  RnnAmdClassScore *scores;
} ClassifyWanted;

/* the staging buffers, with room for the plan's first (largest) wave; the h_* ones are the host sides and stay untouched
 * from a wave's copies to its synchronisation */
typedef struct ClassifyBuffers {
  u8 *h_text, *d_text;
  u8 *h_cls, *d_cls; /* NULL: no text has class bytes */
  unsigned long long *h_off, *d_off;
  int *d_skip;
  double *h_acc, *d_acc; /* [rows][RAMD_CLASSIFY_ACC_WORDS] */
  float *h_state;        /* [rows][H] the wave's states on their way in and out, or NULL */
} ClassifyBuffers;

static void run_wave(const RamdRows *rows, const TextsPlan *plan, int w, const ClassifyBuffers *cb,
                     const ClassifyWanted *want) {
  RamdEngine *e = rows->e;
  const RamdShape *s = &e->sh;
  const TextsWave *wave = &plan->waves[w];
  const int n = wave->nrows;
  const size_t n_out = (size_t)s->output_size, words = RAMD_CLASSIFY_ACC_WORDS(n_out);
  size_t at = 0;
  for (int j = 0; j < n; j++) {
    const int k = plan->order[wave->row0 + j];
    const size_t len = (size_t)(plan->len[wave->row0 + j] - 1); /* (the plan's text is one symbol longer) */
    cb->h_off[j] = at;
    memcpy(cb->h_text + at, want->texts[k], len);
    if (cb->h_cls) {
      if (want->classes[k]) {
        memcpy(cb->h_cls + at, want->classes[k], len);
      } else {
        memset(cb->h_cls + at, CLASSIFY_NO_CLASS, len);
      }
    }
    at += len;
  }
  ramd_h2d(cb->d_text, cb->h_text, at);
  if (cb->h_cls) {
    ramd_h2d(cb->d_cls, cb->h_cls, at);
  }
  ramd_h2d(cb->d_off, cb->h_off, (size_t)n * sizeof(unsigned long long));
  ramd_h2d(cb->d_skip, plan->skip + wave->row0, (size_t)n * sizeof(int));
  HIP_OK(hipMemsetAsync(cb->d_acc, 0, (size_t)n * words * sizeof(double), ramd_stream));
  RamdClassifyStep step = {.text = cb->d_text, .cls = cb->d_cls, .off = cb->d_off, .skip = cb->d_skip, .acc = cb->d_acc,
                           .row0 = rows->r0};
  step.hid0 = ramd_rows_states_in(rows, plan, w, want->h_in, cb->h_state);
  for (int t = 0; t <= wave->steps; t++) {
    step.t_score = t - 1;
    step.a_score = step.a_feed; /* the rows whose symbol t - 1 waits to be scored */
    step.t_feed = t;
    step.a_feed = t < wave->steps ? texts_plan_active(plan, w, t) : 0;
    ramd_launch_classify_step(ramd_stream, s, &e->b, &step);
    step.hid0 = NULL;
    if (step.a_feed) {
      ramd_rows_forward(rows, step.a_feed);
    }
  }
  ramd_d2h(cb->h_acc, cb->d_acc, (size_t)n * words * sizeof(double));
  /* (a row's last forward pass was its last writer: the passes after it had fewer rows) */
  ramd_rows_states_out(rows, n, want->h_out ? cb->h_state : NULL);
  ramd_dsync(); /* the wave's one synchronisation */
  if (want->h_out) {
    texts_states_unpack(plan, w, cb->h_state, s->H, want->h_out);
  }
  for (int j = 0; j < n; j++) {
    const int k = plan->order[wave->row0 + j];
    const double *acc = cb->h_acc + (size_t)j * words;
    memcpy(want->sums + (size_t)k * n_out, acc, n_out * sizeof(double));
    if (want->sumsqs) {
      memcpy(want->sumsqs + (size_t)k * n_out, acc + n_out, n_out * sizeof(double));
    }
    if (want->scores) {
      long long counts[2];
      memcpy(counts, acc + 2 * n_out + 2, sizeof(counts));
      want->scores[k] = (RnnAmdClassScore){.error = acc[2 * n_out], .entropy = acc[2 * n_out + 1], .correct = counts[0],
                                           .count = counts[1]};
    }
  }
}

int rnn_amd_classify_texts(RecurNN *net, const u8 *const *texts, const int *lens, const int *skips,
                           const u8 *const *classes, int n_texts, const float *h_in, float *h_out, double *sums,
                           double *sumsqs, RnnAmdClassScore *scores) {
  if (classify_refused(net, texts, lens, classes, n_texts, sums)) {
    return -1;
  }
  if (n_texts == 0) {
    return 0;
  }
  const size_t n_out = (size_t)net->output_size;
  for (size_t q = 0; q < (size_t)n_texts * n_out; q++) {
    sums[q] = 0.0;
    if (sumsqs) {
      sumsqs[q] = 0.0;
    }
  }
  for (int k = 0; scores && k < n_texts; k++) {
    scores[k] = (RnnAmdClassScore){0};
  }
  TextsPlan plan = {0};
  int *lens1 = malloc((size_t)n_texts * sizeof(int)); /* the plan's lengths: a text of len symbols has len passes */
  if (!lens1) {
    fprintf(stderr, "librecur_amd: " WHO ": out of memory planning %d texts\n", n_texts);
    return -1;
  }
  for (int k = 0; k < n_texts; k++) {
    lens1[k] = lens[k] + 1;
  }
  if (texts_plan_make(&plan, lens1, skips, n_texts, TEXTS_PLAN_WIDTH)) {
    fprintf(stderr, "librecur_amd: " WHO ": out of memory planning %d texts\n", n_texts);
    free(lens1);
    return -1;
  }
  const int filled = ramd_texts_fill_rowless(net, lens1, n_texts, plan.n_rows, h_in, h_out);
  free(lens1);
  if (filled) {
    fprintf(stderr, "librecur_amd: " WHO ": out of memory\n");
    texts_plan_free(&plan);
    return -1;
  }
  if (plan.n_rows == 0) { /* no text has a symbol: no device is asked for */
    return 0;
  }
  int any_class = 0;
  for (int k = 0; classes && k < n_texts; k++) {
    any_class |= lens[k] >= 1 && classes[k] != NULL;
  }
  const ClassifyWanted want = {.texts = texts, .classes = any_class ? classes : NULL, .h_in = h_in, .h_out = h_out,
                               .sums = sums, .sumsqs = sumsqs, .scores = scores};
  const int widest = plan.waves[0].nrows;
  RamdRows rows;
  ramd_rows_open(&rows, net, widest);
  size_t bytes = 0;
  for (int j = 0; j < widest; j++) {
    bytes += (size_t)(plan.len[j] - 1);
  }
  const size_t words = RAMD_CLASSIFY_ACC_WORDS(n_out);
  ClassifyBuffers cb = {0};
  cb.h_text = ramd_rows_host(&rows, bytes);
  cb.d_text = ramd_rows_dev(&rows, bytes);
  if (any_class) {
    cb.h_cls = ramd_rows_host(&rows, bytes);
    cb.d_cls = ramd_rows_dev(&rows, bytes);
  }
  cb.h_off = ramd_rows_host(&rows, (size_t)widest * sizeof(unsigned long long));
  cb.d_off = ramd_rows_dev(&rows, (size_t)widest * sizeof(unsigned long long));
  cb.d_skip = ramd_rows_dev(&rows, (size_t)widest * sizeof(int));
  cb.h_acc = ramd_rows_host(&rows, (size_t)widest * words * sizeof(double));
  cb.d_acc = ramd_rows_dev(&rows, (size_t)widest * words * sizeof(double));
  if (h_in || h_out) {
    cb.h_state = ramd_rows_host(&rows, (size_t)widest * rows.e->sh.H * sizeof(float));
  }
  for (int w = 0; w < plan.n_waves; w++) {
    run_wave(&rows, &plan, w, &cb, &want);
  }
  ramd_rows_close(&rows);
  texts_plan_free(&plan);
  return 0;
}
