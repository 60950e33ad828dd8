/* rows_host.c -- what the batched forward-only calls share on the host (gnu11 C): rnn_amd_run_texts and _trace_texts
 * (texts_api.c), rnn_amd_sample_texts and _continue_texts (sample_api.c), rnn_amd_run_sequences (seqs_api.c),
 * rnn_amd_classify_texts (classify_texts_api.c), rnn_amd_run_automaton (automaton_api.c) and rnn_amd_dream_sequences
 * (dream_api.c) each give every text, sequence or cell a forward-only state row of the engine's
 * own.  Stated once here: what all of them refuse about the net, the net's hidden row for the rows that never reach the
 * device, how a call opens the rows (ramd_rows_open), how start and final states travel between the caller's arrays and
 * the rows (ramd_rows_states_in / _out; which state belongs to which row stays texts_states.h's business), the forward
 * pass of the rows that a step kernel has fed (ramd_rows_forward), and the list of a call's staging buffers, freed in one
 * place (ramd_rows_host / _dev / _close).  The device side of the same calls is kernels_rows.hip. */
#define RAMD_HIP_HOST 1
#include "rnn_host.h"
#include "texts_states.h"

int ramd_texts_net_refused(const char *who, const RecurNN *net, int alphabet_len) {
  if (net->bottom_layer) {
    /* the layer has ONE input buffer for every clone (recur-nn-init.c:345-346; RamdBuffers.blast): "independent clones
     * of the net" is not a state the reference can be in */
    fprintf(stderr, "librecur_amd: %s: the net has a bottom layer, whose one shared input buffer leaves independent "
                    "clones undefined\n", who);
    return -1;
  }
  if (alphabet_len && (alphabet_len < 0 || net->output_size % alphabet_len != 0)) {
    fprintf(stderr, "librecur_amd: %s: %d outputs are not whole heads of %d\n", who, net->output_size, alphabet_len);
    return -1;
  }
  return 0;
}

/* net's hidden row as it stands at this moment, into row[h_size], with neither of net's copies changed: the host's where
 * that is current, else the device's, read and not adopted */
void ramd_texts_net_hidden_row(RecurNN *net, float *row) {
  const RamdPriv *p = ramd_priv(net);
  RamdEngine *e = p->eng;
  if (p->host_valid || !e || !e->dev_ready) {
    memcpy(row, net->hidden_layer, (size_t)net->h_size * sizeof(float));
    return;
  }
  ramd_d2h(row, e->b.hidden + (size_t)ramd_state_row(e, p) * e->sh.H, (size_t)e->sh.H * sizeof(float));
  ramd_dsync();
}

/* h_out of the texts that take no row: their start state, by the host alone unless the net's hidden row is wanted (h_in
 * NULL) and only the device has it.  Returns 0, or -1 out of memory */
int ramd_texts_fill_rowless(RecurNN *net, const int *lens, int n_texts, int n_rows, const float *h_in, float *h_out) {
  if (!h_out || n_rows == n_texts) {
    return 0;
  }
  float *row = NULL;
  if (!h_in) {
    row = malloc((size_t)net->h_size * sizeof(float));
    if (!row) {
      return -1;
    }
    ramd_texts_net_hidden_row(net, row);
  }
  texts_states_fill_rowless(lens, n_texts, h_in, row, net->h_size, net->hidden_size, h_out);
  free(row);
  return 0;
}

void ramd_rows_open(RamdRows *rows, RecurNN *net, int widest) {
  RamdEngine *e = ramd_engine_of(net);
  if (e->scratch_fwd < widest) {
    e->scratch_fwd = widest; /* the image grows once (every net's state survives: ramd_engine_ensure_device) */
  }
  ramd_engine_ensure_device(e);
  ramd_engine_need_dev(e, RNN_AMD_WEIGHTS);
  ramd_stream_need_dev(e, net);
  ramd_set_uniform_idx(e, e->n_streams, 0); /* forward-only rows: no ring position */
  memset(rows, 0, sizeof(*rows));
  rows->e = e;
  rows->r0 = e->sh.Scap + e->n_fwd; /* the engine's scratch rows lie behind the clones' */
  rows->hid0 = e->b.hidden + (size_t)ramd_state_row(e, ramd_priv(net)) * e->sh.H;
  rows->states = e->b.hidden + (size_t)rows->r0 * e->sh.H;
}

const float *ramd_rows_states_in(const RamdRows *rows, const TextsPlan *plan, int w, const float *h_in, float *h_state) {
  if (!h_in) {
    return rows->hid0;
  }
  const RamdShape *s = &rows->e->sh;
  texts_states_pack(plan, w, h_in, NULL, s->H, s->hidden_size, h_state);
  ramd_h2d(rows->states, h_state, (size_t)plan->waves[w].nrows * s->H * sizeof(float));
  return NULL;
}

void ramd_rows_states_out(const RamdRows *rows, int n, float *dst) {
  if (dst) {
    ramd_d2h(dst, rows->states, (size_t)n * rows->e->sh.H * sizeof(float));
  }
}

void ramd_rows_forward(const RamdRows *rows, int nrows) {
  const RamdFwdCall call = {.row0 = rows->r0, .nrows = nrows, .rows_built = 1};
  ramd_launch_forward(ramd_stream, &rows->e->sh, &rows->e->b, &call, NULL, NULL);
}

static void *remember(void **list, int *n, void *p) {
  if (*n == RAMD_ROWS_STAGING) {
    fprintf(stderr, "librecur_amd: a batched call with more than %d staging buffers on one side\n", RAMD_ROWS_STAGING);
    abort();
  }
  return list[(*n)++] = p;
}

void *ramd_rows_host(RamdRows *rows, size_t bytes) { return remember(rows->host, &rows->n_host, ramd_zalloc(bytes)); }

void *ramd_rows_dev(RamdRows *rows, size_t bytes) { return remember(rows->dev, &rows->n_dev, ramd_dev_alloc(bytes)); }

void ramd_rows_close(RamdRows *rows) {
  while (rows->n_dev) {
    ramd_dev_free(rows->dev[--rows->n_dev]);
  }
  while (rows->n_host) {
    free(rows->host[--rows->n_host]);
  }
}
