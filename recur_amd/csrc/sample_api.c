/* sample_api.c -- many texts drawn from one net in one batched device run (gnu11 C): rnn_amd_sample_texts, the
 * generative counterpart of rnn_amd_run_texts (texts_api.c), and rnn_amd_char_confabulate_texts, its character layer.
 * Where rnn_char_confabulate (char_sampling.c) visits the host for every symbol of one net -- the output row comes back,
 * the host draws, the generator goes out again -- these give every text a forward-only state row of the engine's own and
 * a generator of its own in a buffer of the call's, and run the rows together: between two forward passes of the rows
 * there is one launch (k_texts_sample, kernels_loss.hip) that draws each row's next symbol on the device (sample_rule.h)
 * and builds the input rows of the next pass from it.  The net the caller passes is read -- its weights, its hidden row --
 * and not written. */
#define RAMD_HIP_HOST 1
#include "char_host.h"
#include "texts_plan.h"

#define SAMPLE_CHECK_EVERY 64 /* steps between two looks at the rows' done words */

static int sample_texts_refused(const char *who, const RecurNN *net, const int *first, const u64 *seeds, int n_texts,
                                int max_len, int alphabet_len, int head, const void *out, const int *out_lens) {
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
  if (n_texts > 0 && (!first || !seeds || !out || !out_lens)) {
    fprintf(stderr, "librecur_amd: %s: a NULL array for %d texts\n", who, n_texts);
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
  if (n_texts == 0 || max_len == 0) { /* nothing to draw: no device is asked for */
    for (int k = 0; k < n_texts; k++) {
      out_lens[k] = 0;
      if (rng_out) {
        ramd_init_rand64(&rng_out[k], seeds[k]);
      }
    }
    return 0;
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

/* rnn_char_confabulate's passage (char_sampling.c) n_texts times over, side by side: the same symbols-to-text loop under
 * the same room rule, on the symbols of one rnn_amd_sample_texts call */
int rnn_amd_char_confabulate_texts(RecurNN *net, RnnCharAlphabet *a, const u64 *seeds, int n_texts, int char_len, float bias,
                                   int prev_char, int stop_point, char **dest, int byte_len, int *bytes) {
  const char *who = "rnn_amd_char_confabulate_texts";
  if (!net || !a || n_texts < 0 || char_len < 0 || (n_texts > 0 && (!seeds || !dest || !bytes))) {
    fprintf(stderr, "librecur_amd: %s: %d texts of %d characters, or a NULL argument\n", who, n_texts, char_len);
    return -1;
  }
  const int utf8 = (a->flags & RNN_CHAR_FLAG_UTF8) != 0;
  const int room = byte_len - (utf8 ? 5 : 1); /* a symbol may need four bytes, then the NUL */
  if (room <= 0) {
    fprintf(stderr, "insufficient space to confabulate (%d bytes)\n", byte_len);
    for (int k = 0; k < n_texts; k++) {
      if (byte_len > 0) {
        dest[k][0] = 0;
      }
      bytes[k] = 0;
    }
    return 0;
  }
  if (n_texts == 0) {
    return 0;
  }
  int *first = malloc((size_t)n_texts * sizeof(int));
  int *lens = calloc((size_t)n_texts, sizeof(int)); /* (a refused call writes none) */
  u8 *syms = malloc((size_t)n_texts * RAMD_MAX(char_len, 1));
  for (int k = 0; k < n_texts; k++) {
    first[k] = prev_char;
  }
  const int r = rnn_amd_sample_texts(net, first, seeds, n_texts, char_len, bias, stop_point, 0, 0, syms, lens, NULL);
  for (int k = 0; k < n_texts; k++) {
    int used = 0;
    for (int i = 0; i < lens[k] && used < room; i++) {
      used += ramd_put_codepoint(a->points[syms[(size_t)k * char_len + i]], dest[k] + used, utf8);
    }
    dest[k][used] = 0;
    bytes[k] = used;
  }
  free(first);
  free(lens);
  free(syms);
  return r;
}
