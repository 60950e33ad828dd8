/* set_api.c -- the batched API: an RnnAmdSet drives all the streams of a training set (or a set of forward-only
 * clones) through one launch sequence per call (include/recur_amd.h; gnu11 C).  Here: the set's lifecycle and sharding, the
 * forward pass and the opinion calls, the delta call, the resident text, the fused single-net text step and the statistics.
 * The losses between a pass and its delta call are set_loss.c's, whole generations as ONE call and the block trainers
 * set_train.c's; what the three share is declared in set_internal.h.  The presynaptic noise of the next pass is generated
 * ahead by noise_ahead.c (whether a pass may take it: noise_ahead.h); the exchange between ranks that a step may end with
 * is exchange.c's.
 */
#define RAMD_HIP_HOST 1
#include "set_internal.h"

RnnAmdSet *rnn_amd_set_open(RecurNN **nets, int n_nets) {
  if (!nets || n_nets < 1) {
    return NULL;
  }
  RamdEngine *e = ramd_engine_of(nets[0]);
  /* either training streams in rnn_new_training_set order, or forward-only clones
   * (rnn_clone without bptt, e.g. gstrnnca.c's constructors) in creation order */
  int fwd_only = ramd_priv(nets[0])->stream < 0;
  int row0 = fwd_only ? ramd_priv(nets[0])->fwd : ramd_priv(nets[0])->stream;
  for (int j = 0; j < n_nets; j++) {
    RamdPriv *p = ramd_priv(nets[j]);
    int id = fwd_only ? p->fwd : p->stream;
    if (ramd_engine_of(nets[j]) != e || id != row0 + j || (p->stream < 0) != fwd_only) {
      fprintf(stderr, "librecur_amd: rnn_amd_set_open: nets must be one training set in "
                      "rnn_new_training_set order (or forward-only clones in creation order)\n");
      return NULL;
    }
  }
  ramd_engine_ensure_device(e);
  RnnAmdSet *set = ramd_zalloc(sizeof(RnnAmdSet));
  set->eng = e;
  /* the set keeps its own copy of the pointer array: the caller's may be a temporary */
  set->nets = ramd_zalloc(n_nets * sizeof(RecurNN *));
  memcpy(set->nets, nets, n_nets * sizeof(RecurNN *));
  set->n = n_nets;
  set->row0 = row0;
  set->fwd_only = fwd_only;
  set->global_first = 0;
  set->global_count = n_nets;
  set->counts_shard = 0;
  /* A set of ALL the engine's training streams opened inside a group is this rank's shard of the distributed
   * training set: rank r holds global streams [r n, (r + 1) n).  A set of some of them -- the host layers' one-net
   * passes, a validation or side net that one rank alone touches -- stays local: its host draws must not become
   * collectives that the other ranks never enter. */
  if (ramd_dist_active() && !fwd_only && n_nets == e->n_streams) {
    set->global_first = rnn_amd_dist_rank() * n_nets;
    set->global_count = rnn_amd_dist_world() * n_nets;
    set->counts_shard = 1;
    e->sharded_sets++;
    e->sharded = 1;
  }
  return set;
}

/* the engine stays a shard while ANY open set shards it (two sets may be open on one engine and close in any order:
 * ADVICE.md round 4) or it was sharded explicitly (rnn_amd_set_shard, the shard constructor: the nets remain a shard
 * whatever set drives them) */
static void set_unshard(RnnAmdSet *set) {
  RamdEngine *e = set->eng;
  if (set->counts_shard && e->sharded_sets > 0) {
    e->sharded_sets--;
  }
  set->counts_shard = 0;
  e->sharded = e->sharded_sticky || e->sharded_sets > 0;
}

void rnn_amd_set_close(RnnAmdSet *set) {
  if (!set) {
    return;
  }
  ramd_need_host(set->nets[0], RNN_AMD_EVERYTHING);
  set_unshard(set);
  free(set->nets);
  free(set);
}

/* the same without fetching anything: the streams' state stays current on the device only */
void rnn_amd_set_drop(RnnAmdSet *set) {
  if (!set) {
    return;
  }
  set_unshard(set);
  free(set->nets);
  free(set);
}

int rnn_amd_set_size(const RnnAmdSet *set) { return set->n; }

/* for tests and tools (include/recur_amd.h): reads the engine's book-keeping, touches nothing */
int rnn_amd_set_deferred(const RnnAmdSet *set) {
  const RamdEngine *e = set->eng;
  int bits = 0;
  if (e->kept_live && e->kept.slab) bits |= RNN_AMD_DEFERRED_IH_PLANES;
  if (e->kept_live && e->kept.ho_slab) bits |= RNN_AMD_DEFERRED_HO_PLANES;
  if (e->deltas_zero_pending) bits |= RNN_AMD_DEFERRED_CLEAR;
  if (e->err_pending) bits |= RNN_AMD_DEFERRED_IMAGES;
  if (e->top_done && e->top_done_row0 == set->row0 && e->top_done_n == set->n) bits |= RNN_AMD_DEFERRED_TOP_DONE;
  return bits;
}

void rnn_amd_set_shard(RnnAmdSet *set, int global_first, int global_count) {
  if (global_first < 0 || global_first + set->n > global_count) {
    fprintf(stderr, "librecur_amd: rnn_amd_set_shard(%d, %d) for a set of %d streams\n", global_first,
            global_count, set->n);
    abort();
  }
  set->global_first = global_first;
  set->global_count = global_count;
  if (global_count != set->n) {
    set->eng->sharded_sticky = 1;
  } else if (global_first == 0) {
    set->eng->sharded_sticky = 0; /* the whole set again: host draws come from the nets' own generators as before */
  }
  set->eng->sharded = set->eng->sharded_sticky || set->eng->sharded_sets > 0;
}

void rnn_amd_set_dist_all_reduce_deltas(RnnAmdSet *set) {
  RamdEngine *e = set->eng;
  if (!ramd_dist_active()) {
    return;
  }
  ramd_engine_need_dev(e, RNN_AMD_DELTAS);
  /* ih_delta||ho_delta are one allocation (library-owned or the caller's external buffer) */
  const int tev = ramd_timing_begin(ramd_stream, RAMD_T_XCHG);
  rnn_amd_dist_all_reduce(e->b.ih_delta, e->ih_size + e->ho_size);
  ramd_timing_end(ramd_stream, tev);
  ramd_engine_dev_wrote(e, RNN_AMD_DELTAS);
}

/* first state row of the set (forward-only rows sit after the Scap training rows) */
static int set_state_row0(const RnnAmdSet *set) {
  return set->fwd_only ? set->eng->sh.Scap + set->row0 : set->row0;
}

void ramd_set_need_training(const RnnAmdSet *set, const char *what) {
  if (set->fwd_only) {
    fprintf(stderr, "librecur_amd: %s needs a training set (nets with bptt)\n", what);
    abort();
  }
}

void ramd_set_streams_to_dev(RnnAmdSet *set) {
  RamdEngine *e = set->eng;
  int any = 0;
  for (int j = 0; j < set->n; j++) {
    RamdPriv *p = ramd_priv(set->nets[j]);
    if (!p->dev_valid) {
      ramd_stream_copy(e, set->nets[j], 1);
      p->dev_valid = 1;
      any = 1;
    }
  }
  if (any) {
    ramd_dsync();
    ramd_top_done_clear(e);
  }
  if (!set->fwd_only) {
    ramd_push_indices(e, set->row0, set->n);
    ramd_mail_in_flush();
  }
}

void ramd_set_streams_dev_wrote(RnnAmdSet *set) {
  for (int j = 0; j < set->n; j++) {
    RamdPriv *p = ramd_priv(set->nets[j]);
    p->dev_valid = 1;
    p->host_valid = 0;
  }
}

void rnn_amd_set_advance(RnnAmdSet *set) {
  ramd_set_need_training(set, "rnn_amd_set_advance");
  for (int j = 0; j < set->n; j++) {
    ramd_host_advance(set->nets[j]);
  }
  /* the device's copy of the indices follows with the next call's uploads (ramd_push_indices): no
   * launch of its own for rnn_bptt_advance's three integer operations per stream */
}

/* want (RAMD_FWD_*): the whole pass, or stop after the hidden layer's sums and leave them for ramd_launch_text_top /
 * ramd_launch_dense_top; returns what was left (nothing otherwise).  seam (or NULL), with ctx: the multi-head step's offer
 * (set_loss.c), made at the pass's seam where it has one */
RamdHandover ramd_set_forward_seam(RnnAmdSet *set, int mode, const float *d_dense, int ld, int text_i, float *outputs,
                                   int advance, int want, void (*seam)(void *ctx), void *ctx) {
  RamdEngine *e = set->eng;
  ramd_top_done_clear(e);
  ramd_engine_need_dev(e, RNN_AMD_WEIGHTS);
  ramd_set_streams_to_dev(set);
  if (advance) {
    ramd_set_need_training(set, "advancing");
    for (int j = 0; j < set->n; j++) {
      ramd_host_advance(set->nets[j]); /* the device steps its copy inside the assemble kernel */
      e->idx_pushed[set->row0 + j] = set->nets[j]->bptt->index;
    }
  }
  const int r0 = set_state_row0(set);
  if (set->fwd_only) {
    e->b.uniform_idx = -1;
  } else {
    ramd_set_uniform_idx(e, set->row0, set->n);
  }
  if (mode == RAMD_IN_DENSE) {
    e->b.dense_inputs = 1;
  } else if (mode == RAMD_IN_ONE_HOT || mode == RAMD_IN_TEXT) {
    e->b.dense_inputs = 0;
  }
  float noise = set->nets[0]->presynaptic_noise;
  /* values generated ahead for exactly this pass, and nothing has touched the generators since? */
  ramd_noise_ahead_pass(e, r0, set->n, noise);
  for (int j = 1; j < set->n; j++) {
    if (set->nets[j]->presynaptic_noise != noise) {
      fprintf(stderr, "librecur_amd: the nets of a set must share presynaptic_noise\n");
      abort();
    }
  }
  /* (when advancing, the ring index the device stores is the host's, which has just stepped) */
  const RamdFwdCall call = {.row0 = r0, .nrows = set->n, .mode = mode, .dense = d_dense, .ld = ld, .text_i = text_i,
                            .global_first = set->global_first, .global_count = set->global_count, .advance = advance,
                            .noise = noise, .fwd_only = set->fwd_only, .want = want};
  const RamdHandover left = ramd_launch_forward(ramd_stream, &e->sh, &e->b, &call, seam, ctx);
  ramd_noise_ahead_pass_done(e);
  ramd_set_streams_dev_wrote(set);
  if (outputs) {
    ramd_d2h(outputs, e->b.out + (size_t)r0 * e->sh.O, (size_t)set->n * e->sh.O * sizeof(float));
    ramd_dsync();
  }
  return left;
}

void rnn_amd_set_opinion(RnnAmdSet *set, const float *inputs, int ld_inputs, float *outputs) {
  RamdEngine *e = set->eng;
  if (inputs) {
    int w = e->sh.bI ? e->sh.b_in : e->sh.input_size;
    /* (queued: leaves with the ring indices in the forward pass's flush) */
    ramd_upload_rows_q(e->d_dense, inputs, ld_inputs * sizeof(float), w * sizeof(float), set->n, set->fwd_only);
    ramd_set_forward(set, RAMD_IN_DENSE, e->d_dense, w, 0, outputs, 0, RAMD_FWD_WHOLE);
    if (e->sh.bI) {
      /* the layer's one input buffer, shared by every clone, as the per-net loop would leave it:
       * the last stream's inputs (recur-nn.c:88-94) */
      RecurExtraLayer *bl = set->nets[0]->bottom_layer;
      bl->inputs[0] = 1.0f;
      memcpy(bl->inputs + 1, inputs + (size_t)(set->n - 1) * ld_inputs, sizeof(float) * bl->input_size);
    }
  } else {
    ramd_set_forward(set, RAMD_IN_KEEP, NULL, 0, 0, outputs, 0, RAMD_FWD_WHOLE);
  }
}

void rnn_amd_set_one_hot_opinion(RnnAmdSet *set, const int *hot, float *outputs) {
  RamdEngine *e = set->eng;
  ramd_upload(e->b.hot + set_state_row0(set), hot, set->n * sizeof(int));
  ramd_set_forward(set, RAMD_IN_ONE_HOT, NULL, 0, 0, outputs, 0, RAMD_FWD_WHOLE);
}

void rnn_amd_set_put_o_error(RnnAmdSet *set, const float *o_error, int ld) {
  RamdEngine *e = set->eng;
  ramd_top_done_clear(e);
  ramd_set_need_training(set, "rnn_amd_set_put_o_error");
  ramd_set_streams_to_dev(set);
  ramd_upload_rows(e->b.o_error + (size_t)set->row0 * e->sh.O, o_error, ld * sizeof(float), e->sh.O * sizeof(float),
              set->n);
  ramd_set_streams_dev_wrote(set);
}

/* the set calls' active mask on the device (b.active, written by nothing else): uploaded unless these very flags are
 * there already -- the class-group loss sends the flags it returns along with its own uploads, because its caller passes
 * them straight on to the delta call (one launch less per generation).  queued: leaves with the caller's next flush */
void ramd_set_active_mask_to_dev(RamdEngine *e, const u8 *active, int n, int queued) {
  if (e->active_host && e->active_host_n == n && memcmp(e->active_host, active, (size_t)n) == 0) {
    return;
  }
  if (!e->active_host) {
    e->active_host = ramd_zalloc((size_t)e->sh.Scap + 4);
  }
  memcpy(e->active_host, active, (size_t)n);
  e->active_host_n = n;
  if (queued) {
    ramd_upload_q(e->b.active, active, (size_t)n);
  } else {
    ramd_upload(e->b.active, active, (size_t)n); /* (through the mailbox when the set is a whole number of words) */
  }
}

/* may this set call leave its delta sums as planes (RamdEngine.kept)?  Not with a bottom layer (its deltas follow in
 * a launch of their own that accumulates), an exchange between ranks or a caller's delta buffer (both want the sums
 * as such, at once); the workspace is the engine's own, made on first use: eight planes and the rest rows' planes */
static int kept_deltas_ok(RamdEngine *e) {
  static int on = -1;
  if (on < 0) {
    const char *v = getenv("RECUR_AMD_KEEP_DELTAS");
    on = !(v && *v == '0');
  }
  if (!on || e->sh.bI || e->xchg_world || e->delta_external || rnn_amd_dist_world() > 1) {
    return 0;
  }
  if (!e->d_kept_slab) {
    size_t fl = 8 * e->ih_size + (size_t)64 * 128 * e->sh.H;
    if (fl * sizeof(float) > ((size_t)2 << 30)) {
      return 0;
    }
    e->d_kept_slab = ramd_dev_alloc(fl * sizeof(float));
    e->kept_floats = fl;
  }
  return 1;
}

/* dev_ranges: one range list per stream already on the device (range_stride ints apart),
 * instead of the shared host list `ranges`.  dev_active (or NULL, with `active` only): these very flags lie on the device
 * already (rnn_amd_set_classify_steps's per-generation masks) and the launch reads them there instead of b.active; the
 * host copy `active` still drives the book-keeping here: the top launch's mask, the pending images, generation++ */
void ramd_set_calc_deltas(RnnAmdSet *set, int accumulate, RecurErrorRange *ranges, const u8 *active, const u8 *dev_active,
                          unsigned extra_flags, const int *dev_ranges, int range_stride, RamdPendingDelta *defer) {
  RamdEngine *e = set->eng;
  ramd_set_need_training(set, "rnn_amd_set_calc_deltas");
  if (e->deltas_zero_pending) { /* the sum into zeros is the sum */
    accumulate = 0;
    e->deltas_zero_pending = 0;
  }
  ramd_engine_need_dev(e, RNN_AMD_WEIGHTS | (accumulate ? RNN_AMD_DELTAS : 0));
  e->kept_live = 0; /* (summed just now if this call accumulates, otherwise overwritten) */
  if (!defer && !accumulate && kept_deltas_ok(e)) {
    /* leave the sums as planes for the rnn_apply_learning that normally follows (see RamdEngine.kept) */
    memset(&e->kept, 0, sizeof(e->kept));
    e->kept.own_slab = e->d_kept_slab;
    e->kept.own_slab_floats = e->kept_floats;
    defer = &e->kept;
  }
  ramd_set_streams_to_dev(set);
  ramd_push_learn_rates(e, set->row0, set->n);
  const int *d_ranges = dev_ranges ? dev_ranges : ramd_push_ranges(e, ranges);
  const unsigned char *d_active = NULL;
  if (active && dev_active) {
    d_active = dev_active;
  } else if (active) {
    ramd_set_active_mask_to_dev(e, active, set->n, 0);
    d_active = e->b.active;
  }
  if (e->err_pending && d_ranges && e->err_row0 == set->row0 && e->err_nrows == set->n) {
    /* the ranged top backprops keep stale entries of these rows' error images, which have not been rebuilt yet: the
     * launcher sees to it (its per-head form reads them from the planes: no k_err_writeback launch) */
    extra_flags |= RAMD_IMAGES_PENDING;
    e->err_pending = 0;
  } else if (e->err_pending && (d_ranges || e->err_row0 != set->row0 || e->err_nrows != set->n ||
                                (active && memchr(active, 0, (size_t)set->n)))) {
    /* (the same rows, no ranges, every stream: this call's images replace the pending ones -- what they keep of the
     * last run, h_error from h_size on behind a single step, bptt_control_wave has left already.  A stream the mask
     * leaves out keeps its images whole: they are rebuilt first) */
    ramd_err_flush(e);
  }
  if (e->top_done && e->top_done_row0 == set->row0 && e->top_done_n == set->n && !d_ranges &&
      (e->top_done_masked ? (active && e->top_done_mask && memcmp(e->top_done_mask, active, (size_t)set->n) == 0)
                          : !active)) {
    extra_flags |= RAMD_TOP_DONE; /* with the loss (rnn_amd_set_opinion_sigmoid_mse / _grouped_softmax) */
  }
  ramd_top_done_clear(e);
  ramd_set_uniform_idx(e, set->row0, set->n);
  ramd_launch_calc_deltas(ramd_stream, &e->sh, &e->b, set->row0, set->n, accumulate, d_ranges,
                          dev_ranges ? range_stride : 0, d_active,
                          set->nets[0]->flags | extra_flags, defer);
  if (e->sh.bI) {
    if (set->global_count != set->n || e->delta_external) {
      fprintf(stderr, "librecur_amd: a bottom layer cannot be trained on a sharded set: its "
                      "error accumulator runs through the streams in order "
                      "(recur-nn.c:377-382)\n");
      abort();
    }
    ramd_launch_bottom_deltas(ramd_stream, &e->sh, &e->b, set->row0, set->n, accumulate, d_active);
  }
  e->err_pending = 1;
  e->err_row0 = set->row0;
  e->err_nrows = set->n;
  if (defer == &e->kept) {
    e->kept_live = e->kept.slab || e->kept.ho_slab;
  }
  ramd_engine_dev_wrote(e, RNN_AMD_DELTAS);
  ramd_set_streams_dev_wrote(set);
  for (int j = 0; j < set->n; j++) {
    if (!active || active[j]) {
      set->nets[j]->generation++; /* recur-nn.c:765 */
    }
  }
  if (set->nets[0]->log) {
    ramd_log_bptt(e, set->nets[0], set->nets[0]->bptt->min_error_factor);
    ramd_pull_scalars(e, set->row0, 1);
    rnn_log_int(set->nets[0], "generation", set->nets[0]->generation);
  }
}

void rnn_amd_set_calc_deltas(RnnAmdSet *set, int accumulate, RecurErrorRange *ranges,
                             const u8 *active) {
  ramd_set_calc_deltas(set, accumulate, ranges, active, NULL, 0, NULL, 0, NULL);
}

void ramd_set_check_text_pos(RamdEngine *e, int i, int last_ok, const char *what) {
  if (!e->b.text) {
    fprintf(stderr, "librecur_amd: %s without rnn_amd_set_load_text\n", what);
    abort();
  }
  /* the reference's loops run i over [start, len - 1) (charmodel-predict.c:288,
   * charmodel-multi-predict.c:244); the kernels wrap the per-stream offset once, so i
   * itself has to be in range */
  if (i < 0 || i >= e->b.text_len - 1 + last_ok) {
    fprintf(stderr, "librecur_amd: %s: text position %d outside [0, %d)\n", what, i,
            e->b.text_len - 1 + last_ok);
    abort();
  }
}

/* rnn_bptt_advance (optional) + one_hot_opinion of the stream's text symbol, nothing else:
 * rnn_char_multitext_spin's step (charmodel-multi-predict.c:293-297); i may be len - 1 */
void rnn_amd_set_text_opinion(RnnAmdSet *set, int i, int advance) {
  RamdEngine *e = set->eng;
  ramd_set_check_text_pos(e, i, 1, "rnn_amd_set_text_opinion");
  ramd_set_forward(set, RAMD_IN_TEXT, NULL, 0, i, NULL, advance, RAMD_FWD_WHOLE);
}

/* fill_frame's fast_sigmoid_array(answer, answer, n) (gstrnnca.c:813-814) for every net of the
 * set (training or forward-only), then optionally the n_nets x o_size answers to the host */
void rnn_amd_set_sigmoid_outputs(RnnAmdSet *set, int n, float *outputs) {
  RamdEngine *e = set->eng;
  if (n < 1 || n > e->sh.output_size) {
    fprintf(stderr, "librecur_amd: rnn_amd_set_sigmoid_outputs over %d of %d outputs\n", n,
            e->sh.output_size);
    abort();
  }
  ramd_set_streams_to_dev(set);
  const int r0 = set_state_row0(set);
  ramd_launch_sigmoid_outputs(ramd_stream, &e->sh, &e->b, r0, set->n, n);
  ramd_set_streams_dev_wrote(set);
  if (outputs) {
    ramd_d2h(outputs, e->b.out + (size_t)r0 * e->sh.O, (size_t)set->n * e->sh.O * sizeof(float));
    ramd_dsync();
  }
}

void rnn_amd_set_load_text(RnnAmdSet *set, const u8 *text, int len) {
  RamdEngine *e = set->eng;
  if (!text || len < 2) { /* a step reads text[o] and text[o + 1] */
    fprintf(stderr, "librecur_amd: rnn_amd_set_load_text needs at least 2 symbols (got %d)\n", len);
    abort();
  }
  ramd_dsync();
  ramd_dev_free(e->b.text);
  e->b.text = ramd_dev_alloc((size_t)len + 1); /* zeroed: the "next symbol" of the last one */
  ramd_h2d(e->b.text, text, len);
  e->b.text_len = len;
  ramd_dsync();
}

/* The single-net text step of rnn_char_epoch (charmodel-predict.c:312-321) without a host round trip per
 * symbol: rnn_bptt_advance, one_hot_opinion of text[i], net_error_bptt's loss against text[i + 1] (on the
 * device, into the set's statistics) and rnn_bptt_calculate(net, batch_size) -- the top layer updated at once
 * with bptt->momentum, the recurrent layer every batch_size generations (recur-nn.c:919-1019).  For a set of
 * ONE net; the caller sets bptt->momentum as the reference's loop does. */
void rnn_amd_set_char_step_fused(RnnAmdSet *set, int i, unsigned batch_size) {
  RamdEngine *e = set->eng;
  ramd_set_need_training(set, "rnn_amd_set_char_step_fused");
  if (set->n != 1) {
    fprintf(stderr, "librecur_amd: rnn_amd_set_char_step_fused is the single-net path (set of %d)\n", set->n);
    abort();
  }
  ramd_set_check_text_pos(e, i, 0, "rnn_amd_set_char_step_fused");
  RecurNN *net = set->nets[0];
  const RamdShape *s = &e->sh;
  const int j = set->row0;
  const int batched = batch_size > 1;
  unsigned top_done = 0;
  if (ramd_text_top_ok(s)) { /* advance + hidden layer, then output layer, loss and top backprop in one launch */
    const RamdHandover left = ramd_set_forward(set, RAMD_IN_TEXT, NULL, 0, i, NULL, 1, RAMD_FWD_FOR_TEXT_TOP);
    if (!left.top_done) { /* (one stream: always -- the one-launch form takes whole row tiles) */
      ramd_launch_text_top(ramd_stream, s, &e->b, j, 1, left);
    }
    top_done = RAMD_TOP_DONE;
  } else {
    ramd_set_forward(set, RAMD_IN_TEXT, NULL, 0, i, NULL, 1, RAMD_FWD_WHOLE); /* advance + one-hot opinion */
    ramd_launch_softmax_error(ramd_stream, s, &e->b, j, 1);
  }
  int accumulate = batched;
  ramd_deltas_materialize(e); /* a pending rnn_bptt_clear_deltas: this path never writes ho_delta (see calc_deltas_one) */
  ramd_engine_need_dev(e, RNN_AMD_WEIGHTS | RNN_AMD_MOMENTUMS | RNN_AMD_DELTAS);
  ramd_push_learn_rates(e, j, 1);
  if (e->err_pending && (e->err_row0 != j || e->err_nrows != 1)) {
    ramd_err_flush(e);
  }
  ramd_set_uniform_idx(e, j, 1);
  ramd_launch_calc_deltas(ramd_stream, s, &e->b, j, 1, accumulate, NULL, 0, NULL,
                          net->flags | RAMD_NO_HO_DELTA | (batched ? 0 : RAMD_IH_SCALE_IN_RATE) | top_done, NULL);
  ramd_err_after_calc(e, j, 1);
  net->generation++;
  ramd_set_streams_dev_wrote(set);
  ramd_fused_net_update(e, net, j, batch_size);
}

void rnn_amd_set_read_stats(RnnAmdSet *set, RnnAmdStats *stats, int clear) {
  RamdEngine *e = set->eng;
  ramd_set_need_training(set, "rnn_amd_set_read_stats");
  int n = set->n, r0 = set->row0;
  double *d = malloc(4 * n * sizeof(double));
  long long *l = malloc(2 * n * sizeof(long long));
  ramd_d2h(d, e->b.stat_err + r0, n * sizeof(double));
  ramd_d2h(d + n, e->b.stat_ent + r0, n * sizeof(double));
  ramd_d2h(d + 2 * n, e->b.stat_zero + r0, n * sizeof(double));
  ramd_d2h(d + 3 * n, e->b.stat_depth + r0, n * sizeof(double));
  ramd_d2h(l, e->b.stat_correct + r0, n * sizeof(long long));
  ramd_d2h(l + n, e->b.stat_count + r0, n * sizeof(long long));
  ramd_dsync();
  memset(stats, 0, sizeof(*stats));
  for (int j = 0; j < n; j++) {
    stats->error += d[j];
    stats->entropy += d[n + j];
    stats->hidden_zeros += d[2 * n + j];
    stats->bptt_depth_sum += d[3 * n + j];
    stats->correct += l[j];
    stats->count += l[n + j];
  }
  free(d);
  free(l);
  if (clear) {
    HIP_OK(hipMemsetAsync(e->b.stat_err + r0, 0, n * sizeof(double), ramd_stream));
    HIP_OK(hipMemsetAsync(e->b.stat_ent + r0, 0, n * sizeof(double), ramd_stream));
    HIP_OK(hipMemsetAsync(e->b.stat_zero + r0, 0, n * sizeof(double), ramd_stream));
    HIP_OK(hipMemsetAsync(e->b.stat_depth + r0, 0, n * sizeof(double), ramd_stream));
    HIP_OK(hipMemsetAsync(e->b.stat_correct + r0, 0, n * sizeof(long long), ramd_stream));
    HIP_OK(hipMemsetAsync(e->b.stat_count + r0, 0, n * sizeof(long long), ramd_stream));
  }
}

void rnn_amd_set_external_delta(RnnAmdSet *set, void *device_buffer) {
  RamdEngine *e = set->eng;
  float *dst = device_buffer ? (float *)device_buffer : e->delta_own;
  ramd_deltas_materialize(e);
  if (dst != e->b.ih_delta) {
    HIP_OK(hipMemcpyAsync(dst, e->b.ih_delta, (e->ih_size + e->ho_size) * sizeof(float),
                          hipMemcpyDeviceToDevice, ramd_stream));
    ramd_dsync();
    e->b.ih_delta = dst;
    e->b.ho_delta = dst + e->ih_size;
  }
  e->delta_external = device_buffer != NULL;
}
