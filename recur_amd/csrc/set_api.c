/* set_api.c -- the batched API: an RnnAmdSet drives all the streams of a training set (or a set of forward-only
 * clones) through one launch sequence per call (include/recur_amd.h; gnu11 C).  Forward passes, the losses, the delta
 * call, the multi-head and text calls, and the generations as ONE call (set_step).  The presynaptic noise of the next
 * pass is generated ahead by noise_ahead.c (whether a pass may take it: noise_ahead.h); here are only the places where a
 * pass asks for it, where it is offered, and where the loss and the classes are reported.  The exchange between ranks
 * that a step may end with is exchange.c's.
 */
#define RAMD_HIP_HOST 1
#include "rnn_host.h"
#include "parrot_rule.h"
#include "automaton_train_rule.h"
#include "classify_train_rule.h"

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

static void set_streams_to_dev(RnnAmdSet *set) {
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

static void set_streams_dev_wrote(RnnAmdSet *set) {
  for (int j = 0; j < set->n; j++) {
    RamdPriv *p = ramd_priv(set->nets[j]);
    p->dev_valid = 1;
    p->host_valid = 0;
  }
}

void rnn_amd_set_advance(RnnAmdSet *set) {
  RamdEngine *e = set->eng;
  ramd_set_need_training(set, "rnn_amd_set_advance");
  (void)e;
  for (int j = 0; j < set->n; j++) {
    ramd_host_advance(set->nets[j]);
  }
  /* the device's copy of the indices follows with the next call's uploads (ramd_push_indices): no
   * launch of its own for rnn_bptt_advance's three integer operations per stream */
}

/* The multi-head step's offer to generate the next pass's noise between its forward pass and its loss of `classes` heads
 * (noise_ahead.c): made where the pass has its seam -- from the fused hidden layer's end on, beside the output layer and
 * the loss -- or else right behind the pass, and only when the pass took its own noise from a slot.  offered: it has been
 * made, so the loss makes none of its own. */
typedef struct EarlyOffer {
  RnnAmdSet *set;
  int classes, offered;
} EarlyOffer;

static void early_offer(void *ctx) {
  EarlyOffer *o = ctx;
  if (!o->offered && ramd_noise_ahead_adopted(o->set->eng)) {
    ramd_noise_ahead_offer(o->set, o->classes);
    o->offered = 1;
  }
}

/* want (RAMD_FWD_*): the whole pass, or stop after the hidden layer's sums and leave them for ramd_launch_text_top /
 * ramd_launch_dense_top; returns what was left (nothing otherwise).  early (or NULL): the multi-head step's offer, made at
 * the pass's seam where it has one */
static RamdHandover set_forward_seam(RnnAmdSet *set, int mode, const float *d_dense, int ld, int text_i,
                                     float *outputs, int advance, int want, EarlyOffer *early) {
  RamdEngine *e = set->eng;
  ramd_top_done_clear(e);
  ramd_engine_need_dev(e, RNN_AMD_WEIGHTS);
  set_streams_to_dev(set);
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
  const RamdHandover left = ramd_launch_forward(ramd_stream, &e->sh, &e->b, &call, early ? early_offer : NULL, early);
  ramd_noise_ahead_pass_done(e);
  set_streams_dev_wrote(set);
  if (outputs) {
    ramd_d2h(outputs, e->b.out + (size_t)r0 * e->sh.O, (size_t)set->n * e->sh.O * sizeof(float));
    ramd_dsync();
  }
  return left;
}

static RamdHandover set_forward(RnnAmdSet *set, int mode, const float *d_dense, int ld, int text_i,
                                float *outputs, int advance, int want) {
  return set_forward_seam(set, mode, d_dense, ld, text_i, outputs, advance, want, NULL);
}

void rnn_amd_set_opinion(RnnAmdSet *set, const float *inputs, int ld_inputs, float *outputs) {
  RamdEngine *e = set->eng;
  if (inputs) {
    int w = e->sh.bI ? e->sh.b_in : e->sh.input_size;
    /* (queued: leaves with the ring indices in set_forward's flush) */
    ramd_upload_rows_q(e->d_dense, inputs, ld_inputs * sizeof(float), w * sizeof(float), set->n, set->fwd_only);
    set_forward(set, RAMD_IN_DENSE, e->d_dense, w, 0, outputs, 0, RAMD_FWD_WHOLE);
    if (e->sh.bI) {
      /* the layer's one input buffer, shared by every clone, as the per-net loop would leave it:
       * the last stream's inputs (recur-nn.c:88-94) */
      RecurExtraLayer *bl = set->nets[0]->bottom_layer;
      bl->inputs[0] = 1.0f;
      memcpy(bl->inputs + 1, inputs + (size_t)(set->n - 1) * ld_inputs, sizeof(float) * bl->input_size);
    }
  } else {
    set_forward(set, RAMD_IN_KEEP, NULL, 0, 0, outputs, 0, RAMD_FWD_WHOLE);
  }
}

void rnn_amd_set_one_hot_opinion(RnnAmdSet *set, const int *hot, float *outputs) {
  RamdEngine *e = set->eng;
  ramd_upload(e->b.hot + set_state_row0(set), hot, set->n * sizeof(int));
  set_forward(set, RAMD_IN_ONE_HOT, NULL, 0, 0, outputs, 0, RAMD_FWD_WHOLE);
}

void rnn_amd_set_put_o_error(RnnAmdSet *set, const float *o_error, int ld) {
  RamdEngine *e = set->eng;
  ramd_top_done_clear(e);
  ramd_set_need_training(set, "rnn_amd_set_put_o_error");
  set_streams_to_dev(set);
  ramd_upload_rows(e->b.o_error + (size_t)set->row0 * e->sh.O, o_error, ld * sizeof(float), e->sh.O * sizeof(float),
              set->n);
  set_streams_dev_wrote(set);
}

void rnn_amd_set_softmax_error(RnnAmdSet *set, const int *target) {
  RamdEngine *e = set->eng;
  ramd_top_done_clear(e);
  ramd_set_need_training(set, "rnn_amd_set_softmax_error");
  set_streams_to_dev(set);
  if (target) {
    ramd_upload(e->b.target + set->row0, target, set->n * sizeof(int));
  }
  ramd_launch_softmax_error(ramd_stream, &e->sh, &e->b, set->row0, set->n);
  set_streams_dev_wrote(set);
}

/* the set calls' active mask on the device (b.active, written by nothing else): uploaded unless these very flags are
 * there already -- the class-group loss sends the flags it returns along with its own uploads, because its caller passes
 * them straight on to the delta call (one launch less per generation).  queued: leaves with the caller's next flush */
static void active_mask_to_dev(RamdEngine *e, const u8 *active, int n, int queued) {
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
static void set_calc_deltas_masked(RnnAmdSet *set, int accumulate, RecurErrorRange *ranges,
                                   const u8 *active, const u8 *dev_active, unsigned extra_flags, const int *dev_ranges,
                                   int range_stride, RamdPendingDelta *defer) {
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
  set_streams_to_dev(set);
  ramd_push_learn_rates(e, set->row0, set->n);
  const int *d_ranges = dev_ranges ? dev_ranges : ramd_push_ranges(e, ranges);
  const unsigned char *d_active = NULL;
  if (active && dev_active) {
    d_active = dev_active;
  } else if (active) {
    active_mask_to_dev(e, active, set->n, 0);
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
  set_streams_dev_wrote(set);
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

static void set_calc_deltas(RnnAmdSet *set, int accumulate, RecurErrorRange *ranges,
                            const u8 *active, unsigned extra_flags, const int *dev_ranges,
                            int range_stride, RamdPendingDelta *defer) {
  set_calc_deltas_masked(set, accumulate, ranges, active, NULL, extra_flags, dev_ranges, range_stride, defer);
}

void rnn_amd_set_calc_deltas(RnnAmdSet *set, int accumulate, RecurErrorRange *ranges,
                             const u8 *active) {
  set_calc_deltas(set, accumulate, ranges, active, 0, NULL, 0, NULL);
}

/* the staging buffer of the losses' targets and class groups (d_group) has room for `bytes` */
static void group_room(RamdEngine *e, size_t bytes) {
  if (bytes > e->d_group_bytes) {
    ramd_dsync();
    ramd_dev_free(e->d_group);
    e->d_group = ramd_dev_alloc(bytes);
    e->d_group_bytes = bytes;
  }
}

/* The class groups of gstclassify's loss on the device, for its launch: every group lies within the outputs (or the call
 * aborts), then one staging block -- offsets, sizes, targets, then the weights (or NULL) -- whose uploads are queued and
 * leave with the caller's next flush; `inputs` (or NULL): the call's dense input rows, which travel in front of them.
 * trained (or NULL): a stream is trained if any of its groups has a usable target. */
typedef struct ClassGroups {
  const int *offset, *size, *targets;
  const float *weight;
  int largest; /* the largest group's size */
} ClassGroups;

static ClassGroups class_groups_stage(RnnAmdSet *set, const float *inputs, int ld_inputs, int n_groups,
                                      const int *group_offset, const int *group_size, const int *targets,
                                      const float *error_weight, u8 *trained) {
  RamdEngine *e = set->eng;
  const RamdShape *s = &e->sh;
  int largest = 1;
  for (int i = 0; i < n_groups; i++) {
    if (group_offset[i] < 0 || group_size[i] < 1 || group_offset[i] + group_size[i] > s->output_size) {
      fprintf(stderr, "librecur_amd: class group %d (%d + %d) outside the %d outputs\n", i, group_offset[i],
              group_size[i], s->output_size);
      abort();
    }
    largest = RAMD_MAX(largest, group_size[i]);
  }
  const size_t ints = (size_t)2 * n_groups + (size_t)set->n * n_groups;
  group_room(e, ints * sizeof(int) + (error_weight ? (size_t)s->output_size * sizeof(float) : 0));
  int *d = (int *)e->d_group;
  ClassGroups g = {d, d + n_groups, d + 2 * n_groups, NULL, largest};
  if (inputs) {
    ramd_upload_rows_q(e->d_dense, inputs, ld_inputs * sizeof(float), s->input_size * sizeof(float), set->n, 0);
  }
  ramd_upload_q(d, group_offset, n_groups * sizeof(int));
  ramd_upload_q(d + n_groups, group_size, n_groups * sizeof(int));
  ramd_upload_q(d + 2 * n_groups, targets, (size_t)set->n * n_groups * sizeof(int));
  if (error_weight) {
    g.weight = (float *)(d + ints);
    ramd_upload_q((float *)(d + ints), error_weight, (size_t)s->output_size * sizeof(float));
  }
  for (int j = 0; trained && j < set->n; j++) {
    trained[j] = 0;
    for (int i = 0; i < n_groups; i++) {
      int t = targets[(size_t)j * n_groups + i];
      trained[j] |= (t >= 0 && t < group_size[i]);
    }
  }
  return g;
}

/* gstclassify's loss for the whole set (gstclassify.c:2070-2119), see recur_amd.h */
void rnn_amd_set_grouped_softmax_error(RnnAmdSet *set, int n_groups, const int *group_offset,
                                       const int *group_size, const int *targets,
                                       const float *error_weight, u8 *trained) {
  RamdEngine *e = set->eng;
  ramd_set_need_training(set, "rnn_amd_set_grouped_softmax_error");
  ramd_top_done_clear(e);
  set_streams_to_dev(set);
  const ClassGroups g = class_groups_stage(set, NULL, 0, n_groups, group_offset, group_size, targets, error_weight, trained);
  /* the caller hands the flags to rnn_amd_set_calc_deltas next (gstclassify.c:2120-2127): they travel with this call's
   * uploads, and that call finds them in place (active_mask_to_dev) */
  if (trained && set->n % 4 == 0 && !set->fwd_only) {
    active_mask_to_dev(e, trained, set->n, 1);
  }
  ramd_mail_in_flush();
  ramd_launch_grouped_softmax_error(ramd_stream, &e->sh, &e->b, set->row0, set->n, n_groups, g.largest, g.offset, g.size,
                                    g.targets, g.weight, NULL);
  set_streams_dev_wrote(set);
}

/* The multi-head text model for the whole set, per generation: what
 * charmodel-multi-predict.c:244-256 does per net (rnn_bptt_advance, multi_softmax_error
 * with its one_hot_opinion, rnn_bptt_calc_deltas with the error ranges), stream j
 * accumulating on top of stream j - 1.  The loss half leaves o_error and one range list
 * per stream on the device; the deltas half consumes them.  In between the caller may
 * apply the previous batch's deltas, as text_train does (244-252). */
static const int MULTI_RANGE_STRIDE = RAMD_MULTI_RANGE_STRIDE; /* 2 x (64 + 1) ints and the head bits */

static int multi_heads(RamdEngine *e, int alphabet_len) {
  const RamdShape *s = &e->sh;
  int n_classes = alphabet_len > 0 ? s->output_size / alphabet_len : 0;
  if (alphabet_len < 1 || n_classes < 1 || n_classes > 64) {
    fprintf(stderr, "librecur_amd: %d outputs as heads of %d: 1 to 64 heads are supported\n",
            s->output_size, alphabet_len);
    abort();
  }
  if (!e->d_mranges) {
    e->d_mranges = ramd_dev_alloc((size_t)s->Scap * MULTI_RANGE_STRIDE * sizeof(int));
    e->d_mclass = ramd_dev_alloc((size_t)s->Scap * sizeof(int));
  }
  /* the sparse top backprop's partial products, one row of h_size per (stream, head): 53 MB at 256 streams of 50
   * heads and 1024 hidden units; sets too large for that keep the one-GEMM form (k_top_backprop_heads) */
  size_t part = (size_t)s->Scap * n_classes * s->H;
  if (alphabet_len >= 24 && alphabet_len <= 128 && part > e->b.mheads_part_floats && part * sizeof(float) <= ((size_t)2 << 30)) {
    ramd_dev_free(e->b.mheads_part);
    e->b.mheads_part = ramd_dev_alloc(part * sizeof(float));
    e->b.mheads_part_floats = part;
  }
  return n_classes;
}

/* the loss after the opinion: b.target holds each stream's next symbol.  offered: the early offer to generate the next
 * pass's noise has been made (multi_step_deltas) */
static void multi_loss(RnnAmdSet *set, const int *target_class, int alphabet_len, int n_classes,
                       float leakage, int offered) {
  RamdEngine *e = set->eng;
  e->mheads_alen = alphabet_len;
  e->b.mheads_alen = alphabet_len;
  if (target_class) {
    ramd_upload(e->d_mclass + set->row0, target_class, set->n * sizeof(int));
    noise_ahead_classes(&e->ahead, target_class, set->n, n_classes);
  }
  noise_ahead_loss(&e->ahead, n_classes); /* the leak decisions are draws from the streams' generators */
  /* u64 threshold = leakage * UINT64_MAX (charmodel-multi-predict.c:27): float arithmetic */
  float tf = leakage * (float)UINT64_MAX;
  unsigned long long threshold = tf >= 18446744073709551615.0f ? UINT64_MAX : (unsigned long long)tf;
  ramd_launch_multi_softmax_error(ramd_stream, &e->sh, &e->b, set->row0, set->n, alphabet_len, n_classes,
                                  threshold, e->d_mclass + set->row0,
                                  e->d_mranges + (size_t)set->row0 * MULTI_RANGE_STRIDE,
                                  MULTI_RANGE_STRIDE);
  set_streams_dev_wrote(set);
  if (!offered) {
    ramd_noise_ahead_offer(set, 0); /* the next draws are the next forward pass's noise */
  }
}

static void multi_calc_deltas(RnnAmdSet *set, int accumulate, RamdPendingDelta *defer) {
  RamdEngine *e = set->eng;
  ramd_set_need_training(set, "rnn_amd_set_multi_calc_deltas");
  if (!e->d_mranges) {
    fprintf(stderr, "librecur_amd: rnn_amd_set_multi_calc_deltas before any multi-head loss\n");
    abort();
  }
  /* (heads of at least 24 columns: a stream's ranges then lie at least 16 columns apart, see k_top_backprop_heads) */
  set_calc_deltas(set, accumulate, NULL, NULL, e->mheads_alen >= 24 ? RAMD_RANGES_ARE_HEADS : 0,
                  e->d_mranges + (size_t)set->row0 * MULTI_RANGE_STRIDE, MULTI_RANGE_STRIDE, defer);
}
void rnn_amd_set_multi_calc_deltas(RnnAmdSet *set, int accumulate) { multi_calc_deltas(set, accumulate, NULL); }

static void multi_step_deltas(RnnAmdSet *set, const int *hot, const int *next, const int *target_class, int alphabet_len,
                              float leakage, int accumulate, RamdPendingDelta *defer) {
  RamdEngine *e = set->eng;
  ramd_set_need_training(set, "rnn_amd_set_multi_step_deltas");
  int n_classes = multi_heads(e, alphabet_len);
  /* the three small uploads leave with one launch */
  ramd_upload_q(e->b.hot + set->row0, hot, set->n * sizeof(int));
  if (target_class) {
    ramd_upload_q(e->d_mclass + set->row0, target_class, set->n * sizeof(int));
    noise_ahead_classes(&e->ahead, target_class, set->n, n_classes);
  }
  ramd_upload(e->b.target + set->row0, next, set->n * sizeof(int));
  EarlyOffer early = {set, n_classes, 0};
  set_forward_seam(set, RAMD_IN_ONE_HOT, NULL, 0, 0, NULL, 1, RAMD_FWD_WHOLE, &early);
  early_offer(&early); /* (a pass without the seam) */
  multi_loss(set, NULL, alphabet_len, n_classes, leakage, early.offered);
  multi_calc_deltas(set, accumulate, defer);
}
void rnn_amd_set_multi_step_deltas(RnnAmdSet *set, const int *hot, const int *next,
                                   const int *target_class, int alphabet_len, float leakage,
                                   int accumulate) {
  multi_step_deltas(set, hot, next, target_class, alphabet_len, leakage, accumulate, NULL);
}

static void check_text_pos(RamdEngine *e, int i, int last_ok, const char *what) {
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

/* the same from the text on the device: stream j reads text[o] and is scored against
 * text[o + 1], o as in rnn_amd_set_char_step */
void rnn_amd_set_multi_text_loss(RnnAmdSet *set, int i, const int *target_class, int alphabet_len,
                                 float leakage) {
  RamdEngine *e = set->eng;
  ramd_set_need_training(set, "rnn_amd_set_multi_text_loss");
  check_text_pos(e, i, 0, "rnn_amd_set_multi_text_loss");
  int n_classes = multi_heads(e, alphabet_len);
  set_forward(set, RAMD_IN_TEXT, NULL, 0, i, NULL, 1, RAMD_FWD_WHOLE); /* advance + one-hot opinion + b.target */
  multi_loss(set, target_class, alphabet_len, n_classes, leakage, 0);
}

/* rnn_bptt_advance (optional) + one_hot_opinion of the stream's text symbol, nothing else:
 * rnn_char_multitext_spin's step (charmodel-multi-predict.c:293-297); i may be len - 1 */
void rnn_amd_set_text_opinion(RnnAmdSet *set, int i, int advance) {
  RamdEngine *e = set->eng;
  check_text_pos(e, i, 1, "rnn_amd_set_text_opinion");
  set_forward(set, RAMD_IN_TEXT, NULL, 0, i, NULL, advance, RAMD_FWD_WHOLE);
}

/* rnnca's loss on the device (gstrnnca.c:701-714) after rnn_amd_set_opinion: sigmoid of the
 * first n outputs in place, o_error = slope * (target - answer); targets: host [n_nets][ld], or (on_dev) device rows ld
 * floats apart: the gathered rows of rnn_amd_set_automaton_steps.  stats: the row's squared error and a count go into the
 * set's statistics -- only rnn_amd_set_automaton_steps asks for that, the public calls leave the statistics alone */
static void set_sigmoid_mse_error(RnnAmdSet *set, const char *what, const float *targets, int ld, int n, int on_dev,
                                  int stats) {
  RamdEngine *e = set->eng;
  ramd_top_done_clear(e);
  ramd_set_need_training(set, what);
  if (n < 1 || n > e->sh.output_size || ld < n) {
    fprintf(stderr, "librecur_amd: %s over %d of %d outputs (ld %d)\n", what, n, e->sh.output_size, ld);
    abort();
  }
  set_streams_to_dev(set);
  if (!on_dev) {
    size_t bytes = (size_t)set->n * n * sizeof(float);
    group_room(e, bytes);
    ramd_upload_rows(e->d_group, targets, ld * sizeof(float), n * sizeof(float), set->n);
    targets = (const float *)e->d_group;
    ld = n;
  }
  ramd_launch_sigmoid_mse_error(ramd_stream, &e->sh, &e->b, set->row0, set->n, n, targets, ld, stats);
  set_streams_dev_wrote(set);
}

void rnn_amd_set_sigmoid_mse_error(RnnAmdSet *set, const float *targets, int ld, int n) {
  set_sigmoid_mse_error(set, "rnn_amd_set_sigmoid_mse_error", targets, ld, n, 0, 0);
}

/* dense inputs -> hidden layer's sums only (they stay in the workspace for ramd_launch_dense_top); 0 where that launch
 * cannot follow */
static int dense_top_ok(RnnAmdSet *set, const float *inputs) {
  RamdEngine *e = set->eng;
  return inputs && !set->fwd_only && !e->sh.bI && ramd_dense_top_ok(&e->sh) &&
         set->nets[0]->presynaptic_noise == 0.0f && set->nets[0]->bptt;
}

/* on_dev: inputs and targets are device rows (never with a bottom layer: rnn_amd_set_automaton_steps refuses such a set);
 * advance: rnn_bptt_advance first; stats: see set_sigmoid_mse_error */
static void set_opinion_sigmoid_mse(RnnAmdSet *set, const float *inputs, int ld_inputs, const float *targets, int ld, int n,
                                    int on_dev, int advance, int stats) {
  RamdEngine *e = set->eng;
  if (!dense_top_ok(set, inputs) || n < 1 || n > e->sh.output_size || ld < n) {
    if (on_dev) {
      set_forward(set, RAMD_IN_DENSE, inputs, ld_inputs, 0, NULL, advance, RAMD_FWD_WHOLE);
    } else {
      if (advance) {
        rnn_amd_set_advance(set);
      }
      rnn_amd_set_opinion(set, inputs, ld_inputs, NULL);
    }
    set_sigmoid_mse_error(set, "rnn_amd_set_sigmoid_mse_error", targets, ld, n, on_dev, stats);
    return;
  }
  ramd_set_need_training(set, "rnn_amd_set_opinion_sigmoid_mse");
  if (!on_dev) {
    size_t bytes = (size_t)set->n * n * sizeof(float);
    group_room(e, bytes);
    /* inputs and targets leave together with the ring indices (set_forward's flush) */
    ramd_upload_rows_q(e->d_dense, inputs, ld_inputs * sizeof(float), e->sh.input_size * sizeof(float), set->n, 0);
    ramd_upload_rows_q(e->d_group, targets, ld * sizeof(float), n * sizeof(float), set->n, 0);
    inputs = e->d_dense;
    ld_inputs = e->sh.input_size;
    targets = (const float *)e->d_group;
    ld = n;
  }
  const RamdHandover left = set_forward(set, RAMD_IN_DENSE, inputs, ld_inputs, 0, NULL, advance, RAMD_FWD_FOR_DENSE_TOP);
  if (!ramd_launch_dense_top(ramd_stream, &e->sh, &e->b, set->row0, set->n, left, targets, ld, n, 0, NULL, NULL, NULL, NULL,
                             stats, NULL)) {
    fprintf(stderr, "librecur_amd: rnn_amd_set_opinion_sigmoid_mse: the top launch declined a shape it had accepted\n");
    abort();
  }
  set_streams_dev_wrote(set);
  ramd_top_done_set(e, set->row0, set->n, 0);
}

void rnn_amd_set_opinion_sigmoid_mse(RnnAmdSet *set, const float *inputs, int ld_inputs, const float *targets, int ld,
                                     int n) {
  set_opinion_sigmoid_mse(set, inputs, ld_inputs, targets, ld, n, 0, 0, 0);
}

/* Parrot's loss (train_net, gstparrot.c:464-477; parrot_rule.h).  The rows of inputs and targets are the caller's host
 * rows, or (on_dev) lie on the device already, ld floats apart: the many-step call's block of frames */
/* what every public call checks once, up front (the static forms below take checked arguments): a training set, targets,
 * 1 <= n <= output_size and rows of at least n floats */
static void tanh_check(const RnnAmdSet *set, const char *what, const float *targets, int ld, int n) {
  ramd_set_need_training(set, what);
  if (!targets || n < 1 || n > set->eng->sh.output_size || ld < n) {
    fprintf(stderr, "librecur_amd: %s: targets %p over %d of %d outputs (ld %d)\n", what, (const void *)targets, n,
            set->eng->sh.output_size, ld);
    abort();
  }
}

static void set_tanh_error(RnnAmdSet *set, const float *targets, int ld, int n, int on_dev) {
  RamdEngine *e = set->eng;
  ramd_top_done_clear(e);
  set_streams_to_dev(set);
  if (!on_dev) {
    group_room(e, (size_t)set->n * n * sizeof(float));
    ramd_upload_rows(e->d_group, targets, ld * sizeof(float), n * sizeof(float), set->n);
    targets = (const float *)e->d_group;
    ld = n;
  }
  ramd_launch_tanh_mse_error(ramd_stream, &e->sh, &e->b, set->row0, set->n, n, targets, ld);
  set_streams_dev_wrote(set);
}

void rnn_amd_set_tanh_error(RnnAmdSet *set, const float *targets, int ld, int n) {
  tanh_check(set, "rnn_amd_set_tanh_error", targets, ld, n);
  set_tanh_error(set, targets, ld, n, 0);
}

static int dense_top_tanh_ok(RnnAmdSet *set, const float *inputs) {
  RamdEngine *e = set->eng;
  return inputs && !set->fwd_only && !e->sh.bI && ramd_dense_top_tanh_ok(&e->sh) &&
         set->nets[0]->presynaptic_noise == 0.0f && set->nets[0]->bptt;
}

/* (advance: rnn_bptt_advance first, as train_net does) */
static void set_opinion_tanh_error(RnnAmdSet *set, const float *inputs, int ld_inputs, const float *targets, int ld, int n,
                                   int on_dev, int advance) {
  RamdEngine *e = set->eng;
  if (!dense_top_tanh_ok(set, inputs)) {
    if (on_dev) { /* (never with a bottom layer: rnn_amd_set_dense_steps_tanh keeps such a set's frames on the host) */
      set_forward(set, RAMD_IN_DENSE, inputs, ld_inputs, 0, NULL, advance, RAMD_FWD_WHOLE);
    } else {
      if (advance) {
        rnn_amd_set_advance(set);
      }
      rnn_amd_set_opinion(set, inputs, ld_inputs, NULL);
    }
    set_tanh_error(set, targets, ld, n, on_dev);
    return;
  }
  if (!on_dev) {
    group_room(e, (size_t)set->n * n * sizeof(float));
    /* inputs and targets leave together with the ring indices (set_forward's flush) */
    ramd_upload_rows_q(e->d_dense, inputs, ld_inputs * sizeof(float), e->sh.input_size * sizeof(float), set->n, 0);
    ramd_upload_rows_q(e->d_group, targets, ld * sizeof(float), n * sizeof(float), set->n, 0);
    inputs = e->d_dense;
    ld_inputs = e->sh.input_size;
    targets = (const float *)e->d_group;
    ld = n;
  }
  const RamdHandover left = set_forward(set, RAMD_IN_DENSE, inputs, ld_inputs, 0, NULL, advance, RAMD_FWD_FOR_DENSE_TOP);
  if (!ramd_launch_dense_top_tanh(ramd_stream, &e->sh, &e->b, set->row0, set->n, left, targets, ld, n)) {
    fprintf(stderr, "librecur_amd: rnn_amd_set_opinion_tanh_error: the top launch declined a shape it had accepted\n");
    abort();
  }
  set_streams_dev_wrote(set);
  ramd_top_done_set(e, set->row0, set->n, 0);
}

void rnn_amd_set_opinion_tanh_error(RnnAmdSet *set, const float *inputs, int ld_inputs, const float *targets, int ld,
                                    int n) {
  tanh_check(set, "rnn_amd_set_opinion_tanh_error", targets, ld, n);
  set_opinion_tanh_error(set, inputs, ld_inputs, targets, ld, n, 0, 0);
}

void rnn_amd_set_opinion_grouped_softmax(RnnAmdSet *set, const float *inputs, int ld_inputs, int n_groups,
                                         const int *group_offset, const int *group_size, const int *targets,
                                         const float *error_weight, u8 *trained) {
  RamdEngine *e = set->eng;
  const RamdShape *s = &e->sh;
  if (!dense_top_ok(set, inputs) || !trained || set->n % 4 != 0) {
    rnn_amd_set_opinion(set, inputs, ld_inputs, NULL);
    rnn_amd_set_grouped_softmax_error(set, n_groups, group_offset, group_size, targets, error_weight, trained);
    return;
  }
  ramd_set_need_training(set, "rnn_amd_set_opinion_grouped_softmax");
  const ClassGroups g = class_groups_stage(set, inputs, ld_inputs, n_groups, group_offset, group_size, targets, error_weight,
                                           trained);
  active_mask_to_dev(e, trained, set->n, 1); /* (for the delta call that follows: travels with the rest) */
  const RamdHandover left = set_forward(set, RAMD_IN_DENSE, e->d_dense, s->input_size, 0, NULL, 0, RAMD_FWD_FOR_DENSE_TOP);
  if (!ramd_launch_dense_top(ramd_stream, s, &e->b, set->row0, set->n, left, NULL, 0, 0, n_groups, g.offset, g.size,
                             g.targets, g.weight, 0, NULL)) {
    fprintf(stderr, "librecur_amd: rnn_amd_set_opinion_grouped_softmax: the top launch declined a shape it had accepted\n");
    abort();
  }
  set_streams_dev_wrote(set);
  ramd_top_done_set(e, set->row0, set->n, 1);
  if (!e->top_done_mask) {
    e->top_done_mask = ramd_zalloc((size_t)e->sh.Scap + 4);
  }
  memcpy(e->top_done_mask, trained, (size_t)set->n); /* (a copy of its own: active_host follows whatever mask is sent next) */
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
  set_streams_to_dev(set);
  const int r0 = set_state_row0(set);
  ramd_launch_sigmoid_outputs(ramd_stream, &e->sh, &e->b, r0, set->n, n);
  set_streams_dev_wrote(set);
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

static void char_step_deltas(RnnAmdSet *set, int i, RamdPendingDelta *defer) {
  RamdEngine *e = set->eng;
  check_text_pos(e, i, 0, "rnn_amd_set_char_step");
  if (ramd_text_top_ok(&e->sh)) {
    /* advance + hidden layer, then output layer, loss and top backprop in one launch */
    const RamdHandover left = set_forward(set, RAMD_IN_TEXT, NULL, 0, i, NULL, 1, RAMD_FWD_FOR_TEXT_TOP);
    ramd_noise_ahead_offer(set, 0); /* no draws between this pass's noise and the next one's */
    ramd_launch_text_top(ramd_stream, &e->sh, &e->b, set->row0, set->n, left);
    set_calc_deltas(set, 0, NULL, NULL, RAMD_TOP_DONE, NULL, 0, defer);
  } else {
    set_forward(set, RAMD_IN_TEXT, NULL, 0, i, NULL, 1, RAMD_FWD_WHOLE); /* advance + one-hot opinion */
    ramd_noise_ahead_offer(set, 0);
    ramd_launch_softmax_error(ramd_stream, &e->sh, &e->b, set->row0, set->n);
    set_calc_deltas(set, 0, NULL, NULL, 0, NULL, 0, defer);
  }
}

void rnn_amd_set_char_step_deltas(RnnAmdSet *set, int i) { char_step_deltas(set, i, NULL); }

/* With ONE rank the sum over the ranks is the rank's own sum and the sharded update is the whole update: the exchange
 * step -- the all-reduce, or the barriers and the peer-pointer update kernel -- is skipped and the generation is the
 * plain one (one-rank cost of either exchange path: 0; round 4: +4.8 us through RCCL, +11 us kernel-issued).
 * RECUR_AMD_DIST_ONE_RANK_EXCHANGE=1 keeps the exchange step in (tests and `bench.py --dist` exercise it on one GPU). */
static int one_rank_exchange_forced(void) {
  static int on = -1;
  if (on < 0) {
    const char *v = getenv("RECUR_AMD_DIST_ONE_RANK_EXCHANGE");
    on = v && *v == '1';
  }
  return on;
}

/* what a one-call generation does before its update: the text step (symbol i of the resident text), or a dense-input
 * generation with rnnca's loss (rnn_amd_set_dense_step_sigmoid_mse) */
typedef struct {
  int i;                /* text position, or -1: dense, or -2: the multi-head step */
  const float *inputs;  /* dense: [n][ld_inputs], the caller's host rows (with on_dev: device rows) */
  int ld_inputs;
  const float *targets; /* [n][ld], host rows or (on_dev) device rows: the first n_targets outputs */
  int ld, n_targets;
  int loss;             /* dense: STEP_LOSS_SIGMOID (rnnca's) or STEP_LOSS_TANH (parrot's) */
  int advance;          /* dense: rnn_bptt_advance in front (parrot's train_net; rnn_amd_set_automaton_steps's `advance`) */
  int on_dev;           /* dense: inputs and targets are device rows (the many-step calls' blocks) */
  int stats;            /* dense, rnnca's: the squared error into the statistics (rnn_amd_set_automaton_steps alone) */
  /* the multi-head step (rnn_amd_set_multi_step_deltas's arguments) */
  const int *hot, *next, *target_class;
  int alphabet_len;
  float leakage;
} StepSpec;
enum { STEP_LOSS_SIGMOID = 0, STEP_LOSS_TANH = 1 };

static void step_deltas(RnnAmdSet *set, const StepSpec *sp, RamdPendingDelta *defer) {
  if (sp->i >= 0) {
    char_step_deltas(set, sp->i, defer);
  } else if (sp->i == -2) {
    multi_step_deltas(set, sp->hot, sp->next, sp->target_class, sp->alphabet_len, sp->leakage, 0, defer);
  } else if (sp->loss == STEP_LOSS_TANH) {
    set_opinion_tanh_error(set, sp->inputs, sp->ld_inputs, sp->targets, sp->ld, sp->n_targets, sp->on_dev, sp->advance);
    set_calc_deltas(set, 0, NULL, NULL, 0, NULL, 0, defer);
  } else {
    set_opinion_sigmoid_mse(set, sp->inputs, sp->ld_inputs, sp->targets, sp->ld, sp->n_targets, sp->on_dev, sp->advance,
                            sp->stats);
    set_calc_deltas(set, 0, NULL, NULL, 0, NULL, 0, defer);
  }
}

static void set_step(RnnAmdSet *set, const StepSpec *sp, int learning_style, float momentum) {
  if (set->eng->xchg_world > 1 || (set->eng->xchg_world == 1 && one_rank_exchange_forced())) {
    /* deltas -> (barrier) -> sharded update with the sum over the ranks in it -> (barrier) */
    step_deltas(set, sp, NULL);
    rnn_amd_set_apply_exchange(set, learning_style, momentum);
    return;
  }
  /* the deltas go straight from the GEMM's K slabs into the update (and into ih_delta) when
   * nothing can look at them in between: library-owned storage, no log on the prototype */
  RamdPendingDelta pend = {0};
  const int dist = ramd_dist_active() && (rnn_amd_dist_world() > 1 || one_rank_exchange_forced());
  int fuse = !set->eng->delta_external && !set->nets[0]->log && !dist;
  if (dist) {
    ramd_halves_seen = 0;
    ramd_set_delta_half_hook(ramd_delta_half_ready, set->eng);
  }
  float mw, rate, ho_rate;
  const int method = ramd_update_rule(set->nets[0]->bptt, learning_style, momentum, &mw, &rate, &ho_rate);
  if (fuse && !set->eng->sh.bI && (method == RNN_MOMENTUM_WEIGHTED || method == RNN_ADAGRAD)) {
    /* the momentum rule (recur-nn.c:482-487, 653-676) or ADAGRAD (518-524, the multi-head trainer's rule): the
     * weight-delta GEMM may carry the update out in its own epilogue (kernels_bptt.hip: k_delta_direct), with the rates
     * and weights ramd_apply_learning would use (ADAGRAD's arithmetic reads neither the momentum nor its weight) */
    _Static_assert(RNN_MOMENTUM_WEIGHTED == 0 && RNN_ADAGRAD == 4, "RamdPendingDelta.fuse_method takes these two as they are");
    ramd_engine_need_dev(set->eng, RNN_AMD_WEIGHTS | RNN_AMD_MOMENTUMS);
    pend.fuse_want = 1;
    pend.fuse_method = method;
    pend.fuse_rate = rate;
    pend.fuse_ho_rate = ho_rate;
    pend.fuse_momentum = momentum;
    pend.fuse_mw = mw;
  }
  step_deltas(set, sp, fuse ? &pend : NULL);
  if (pend.fuse_done) { /* weights and momentum are updated, the delta arrays hold the sums */
    ramd_engine_dev_wrote(set->eng, RNN_AMD_WEIGHTS | RNN_AMD_MOMENTUMS | RNN_AMD_DELTAS);
    return;
  }
  if (dist) {
    /* the one exchange step of the path: this rank's deltas become the sum over all ranks'
     * streams (recur-nn.c:724-739 distributed), then the identical update everywhere */
    ramd_set_delta_half_hook(NULL, NULL);
    if (ramd_halves_seen == 3) { /* both halves are on their way: the update waits for them */
      HIP_OK(hipStreamWaitEvent(ramd_stream, ramd_half_summed[0], 0));
      HIP_OK(hipStreamWaitEvent(ramd_stream, ramd_half_summed[1], 0));
    } else { /* a shape the two-halves form does not take: one all-reduce behind the deltas */
      const int tev = ramd_timing_begin(ramd_stream, RAMD_T_XCHG);
      rnn_amd_dist_all_reduce(set->eng->b.ih_delta, set->eng->ih_size + set->eng->ho_size);
      ramd_timing_end(ramd_stream, tev);
    }
  }
  ramd_apply_learning(set->nets[0], learning_style, momentum, (pend.slab || pend.ho_slab) ? &pend : NULL, NULL);
}

/* the multi-head generation as ONE call: rnn_amd_set_multi_step_deltas (accumulate 0) + rnn_apply_learning -- knowing the
 * update that follows, the weight-delta GEMM carries it out in its own epilogue where the rule is ADAGRAD (the trainer's)
 * or the momentum rule: no optimiser launch (17 us of configs[3]'s 340) */
void rnn_amd_set_multi_step(RnnAmdSet *set, const int *hot, const int *next, const int *target_class, int alphabet_len,
                            float leakage, int learning_style, float momentum) {
  StepSpec sp = {.i = -2, .hot = hot, .next = next, .target_class = target_class, .alphabet_len = alphabet_len,
                 .leakage = leakage};
  set_step(set, &sp, learning_style, momentum);
}

void rnn_amd_set_char_step(RnnAmdSet *set, int i, int learning_style, float momentum) {
  StepSpec sp = {.i = i};
  set_step(set, &sp, learning_style, momentum);
}

/* rnnca's maybe_learn for every trainer (gstrnnca.c:693-740) as one call: see recur_amd.h */
void rnn_amd_set_dense_step_sigmoid_mse(RnnAmdSet *set, const float *inputs, int ld_inputs, const float *targets, int ld,
                                        int n, int learning_style, float momentum) {
  if (!inputs) {
    fprintf(stderr, "librecur_amd: rnn_amd_set_dense_step_sigmoid_mse needs the inputs\n");
    abort();
  }
  rnn_bptt_clear_deltas(set->nets[0]); /* (lazy: the delta call below simply does not accumulate) */
  StepSpec sp = {.i = -1, .inputs = inputs, .ld_inputs = ld_inputs, .targets = targets, .ld = ld, .n_targets = n,
                 .loss = STEP_LOSS_SIGMOID};
  set_step(set, &sp, learning_style, momentum);
}

/* parrot's maybe_learn for every channel at once (gstparrot.c:464-477, 487-554): see recur_amd.h */
static void dense_step_tanh(RnnAmdSet *set, const float *inputs, int ld_inputs, const float *targets, int ld, int n,
                            int on_dev, int learning_style, float momentum) {
  rnn_bptt_clear_deltas(set->nets[0]); /* (lazy: the delta call simply does not accumulate) */
  StepSpec sp = {.i = -1, .inputs = inputs, .ld_inputs = ld_inputs, .targets = targets, .ld = ld, .n_targets = n,
                 .loss = STEP_LOSS_TANH, .advance = 1, .on_dev = on_dev};
  set_step(set, &sp, learning_style, momentum);
}

void rnn_amd_set_dense_step_tanh(RnnAmdSet *set, const float *inputs, int ld_inputs, const float *targets, int ld, int n,
                                 int learning_style, float momentum) {
  tanh_check(set, "rnn_amd_set_dense_step_tanh", targets, ld, n);
  if (!inputs || ld_inputs < set->eng->sh.input_size) {
    fprintf(stderr, "librecur_amd: rnn_amd_set_dense_step_tanh needs inputs (ld %d for %d)\n", ld_inputs,
            set->eng->sh.input_size);
    abort();
  }
  dense_step_tanh(set, inputs, ld_inputs, targets, ld, n, 0, learning_style, momentum);
}

/* n_steps of them from one block of frames, frame t + 1 being generation t's target and generation t + 1's input: the
 * block goes up once, the generations read their rows where they lie */
void rnn_amd_set_dense_steps_tanh(RnnAmdSet *set, const float *frames, int ld, int n_steps, int n, int learning_style,
                                  float momentum, int condition) {
  RamdEngine *e = set->eng;
  ramd_set_need_training(set, "rnn_amd_set_dense_steps_tanh");
  const int refusal = parrot_block_refusal(frames != NULL, n_steps, ld, e->sh.input_size, n, e->sh.output_size);
  if (refusal) { /* (the rule is parrot_rule.h's, where it is asked without a device) */
    fprintf(stderr, "librecur_amd: rnn_amd_set_dense_steps_tanh: %s (%d steps from frames %p of ld %d; %d inputs, %d of %d outputs)\n",
            parrot_block_refusal_text(refusal), n_steps, (const void *)frames, ld, e->sh.input_size, n, e->sh.output_size);
    abort();
  }
  const size_t frame = (size_t)set->n * ld;
  /* (a bottom layer keeps a host copy of the last stream's inputs per generation, rnn_amd_set_opinion: such a set takes
   * its rows from the host, generation by generation) */
  const int on_dev = !e->sh.bI;
  const float *base = frames;
  if (on_dev) {
    const size_t bytes = (size_t)(n_steps + 1) * frame * sizeof(float);
    ramd_engine_ensure_device(e);
    if (bytes > e->d_frames_bytes) {
      ramd_dsync(); /* (an earlier block's generations may still be reading the old one) */
      ramd_dev_free(e->d_frames);
      e->d_frames = ramd_dev_alloc(bytes);
      e->d_frames_bytes = bytes;
    }
    ramd_upload(e->d_frames, frames, bytes);
    base = e->d_frames;
  }
  for (int t = 0; t < n_steps; t++) {
    dense_step_tanh(set, base + (size_t)t * frame, ld, base + (size_t)(t + 1) * frame, ld, n, on_dev, learning_style,
                    momentum);
    if (condition) {
      rnn_condition_net(set->nets[0]); /* gstparrot.c:544-545: behind the update */
    }
  }
}

/* rnnca's trainer over a block of a film (gstrnnca.c:669-750; automaton_train_rule.h): the film, the positions and the
 * offset lists go up once, one launch gathers every generation's input and target rows from the film's bytes, and the
 * generations read their rows where they lie: see recur_amd.h */
static size_t automaton_room(size_t *at, size_t bytes) { /* -> the offset of `bytes` more, 256-byte aligned */
  const size_t here = *at;
  *at = (here + bytes + 255) & ~(size_t)255;
  return here;
}

void rnn_amd_set_automaton_steps(RnnAmdSet *set, const RnnAmdAutomaton *ca, const u8 *frames, const int *xy, int xy_per_step,
                                 int n_steps, int advance, int learning_style, float momentum, float momentum_soft_start,
                                 int condition) {
  AutomatonRule g = {0};
  if (ca) {
    g = (AutomatonRule){ca->width, ca->height, ca->offsets_y, ca->len_y, ca->offsets_c, ca->len_c, ca->len_pos, ca->edges};
  }
  RamdEngine *e = set ? set->eng : NULL;
  const int refusal = automaton_block_refusal(set != NULL, ca ? &g : NULL, frames != NULL, xy, xy_per_step, n_steps,
                                              set ? set->n : 0, e ? e->sh.input_size : 0, e ? e->sh.output_size : 0,
                                              e ? e->sh.bI : 0);
  if (refusal) { /* (the rule is automaton_train_rule.h's, where it is asked without a device) */
    fprintf(stderr, "librecur_amd: rnn_amd_set_automaton_steps: %s (%d steps of %d trainers on a grid of %d x %d)\n",
            automaton_block_refusal_text(refusal), n_steps, set ? set->n : 0, g.width, g.height);
    abort();
  }
  ramd_set_need_training(set, "rnn_amd_set_automaton_steps");
  const int n = set->n, in = e->sh.input_size;
  const size_t cells = (size_t)g.width * g.height;
  const size_t film = ((size_t)n_steps + 1) * 3 * cells, n_xy = 2 * (size_t)(xy_per_step ? n_steps : 1) * n;
  const size_t n_offy = 2 * (size_t)g.len_y, n_offc = 2 * (size_t)g.len_c;
  size_t bytes = 0;
  const size_t at_film = automaton_room(&bytes, film);
  const size_t at_xy = automaton_room(&bytes, n_xy * sizeof(int));
  const size_t at_off = automaton_room(&bytes, (n_offy + n_offc) * sizeof(int));
  const size_t at_rows = automaton_room(&bytes, (size_t)n_steps * n * in * sizeof(float));
  const size_t at_targets = automaton_room(&bytes, (size_t)n_steps * n * 3 * sizeof(float));
  ramd_engine_ensure_device(e);
  if (bytes > e->d_automaton_bytes) {
    ramd_dsync(); /* (an earlier block's generations may still be reading the old one) */
    ramd_dev_free(e->d_automaton);
    e->d_automaton = ramd_dev_alloc(bytes);
    e->d_automaton_bytes = bytes;
  }
  char *base = e->d_automaton;
  int *d_off = (int *)(base + at_off);
  ramd_upload_q(base + at_xy, xy, n_xy * sizeof(int));
  ramd_upload_q(d_off, g.offsets_y, n_offy * sizeof(int));
  ramd_upload_q(d_off + n_offy, g.offsets_c, n_offc * sizeof(int));
  ramd_upload(base + at_film, frames, film);
  g.offsets_y = d_off;
  g.offsets_c = d_off + n_offy;
  const RamdAutomatonTrainRows gather = {.g = g, .frames = (const u8 *)(base + at_film), .xy = (const int *)(base + at_xy),
                                         .xy_per_step = xy_per_step, .n_steps = n_steps, .n = n, .input_size = in,
                                         .rows = (float *)(base + at_rows), .targets = (float *)(base + at_targets)};
  ramd_launch_automaton_train_rows(ramd_stream, &gather);
  for (int t = 0; t < n_steps; t++) {
    rnn_bptt_clear_deltas(set->nets[0]); /* (lazy: the delta call simply does not accumulate) */
    const StepSpec sp = {.i = -1, .inputs = gather.rows + (size_t)t * n * in, .ld_inputs = in,
                         .targets = gather.targets + (size_t)t * n * 3, .ld = 3, .n_targets = 3, .loss = STEP_LOSS_SIGMOID,
                         .advance = advance != 0, .on_dev = 1, .stats = 1};
    set_step(set, &sp, learning_style, automaton_train_momentum(set->nets[0]->generation, momentum, momentum_soft_start));
    if (condition) {
      rnn_condition_net(set->nets[0]); /* gstrnnca.c:739: behind the update */
    }
  }
}

/* gstclassify's trainer over a block of windows (maybe_learn, gstclassify.c:2180-2257; classify_train_rule.h): see
 * recur_amd.h.  One generation from the caller's host rows, the gate decided by reading the summed error back: what the
 * block call does where the block cannot stay on the device (a bottom layer's host copy of its inputs, noise drawn in
 * front of every pass, an exchange or a group of ranks behind every update).  trains: room for a flag per stream */
static void classify_generation_host(RnnAmdSet *set, const float *features, int ld, const int *targets, int n_groups,
                                     const int *group_offset, const int *group_size, const float *error_weight,
                                     int learning_style, float momentum_soft_start, int condition, u8 *trains) {
  RecurNN *net = set->nets[0];
  rnn_bptt_clear_deltas(net);
  RnnAmdStats before, after;
  const int together = net->presynaptic_noise == 0.0f; /* (a noisy pass draws first, as in train_channel) */
  if (!together) {
    rnn_amd_set_opinion(set, features, ld, NULL);
  }
  rnn_amd_set_read_stats(set, &before, 0);
  if (together) {
    rnn_amd_set_opinion_grouped_softmax(set, features, ld, n_groups, group_offset, group_size, targets, error_weight, trains);
  } else {
    rnn_amd_set_grouped_softmax_error(set, n_groups, group_offset, group_size, targets, error_weight, trains);
  }
  const int any = memchr(trains, 1, (size_t)set->n) != NULL;
  if (any) {
    rnn_amd_set_calc_deltas(set, 1, NULL, trains); /* adds to the cleared deltas */
  }
  rnn_amd_set_advance(set);
  if (any) {
    rnn_amd_set_read_stats(set, &after, 0);
    if (after.error - before.error != 0.0) { /* the reference's `if (err_sum)` */
      rnn_apply_learning(net, learning_style,
                         rnn_calculate_momentum_soft_start(net->generation, net->bptt->momentum, momentum_soft_start));
    }
  }
  if (condition) {
    rnn_condition_net(net);
  }
}

void rnn_amd_set_classify_steps(RnnAmdSet *set, const float *features, int ld, const int *targets, int n_steps, int n_groups,
                                const int *group_offset, const int *group_size, const float *error_weight,
                                int learning_style, float momentum_soft_start, int condition) {
  if (!set) {
    fprintf(stderr, "librecur_amd: rnn_amd_set_classify_steps without a set\n");
    abort();
  }
  RamdEngine *e = set->eng;
  ramd_set_need_training(set, "rnn_amd_set_classify_steps");
  const int width = e->sh.bI ? e->sh.b_in : e->sh.input_size; /* (a bottom layer takes the features) */
  const int refusal = classify_block_refusal(features != NULL, targets != NULL, n_steps, ld, width, n_groups, group_offset,
                                             group_size, e->sh.output_size);
  if (refusal) { /* (the rule is classify_train_rule.h's, where it is asked without a device) */
    fprintf(stderr, "librecur_amd: rnn_amd_set_classify_steps: %s (%d steps, rows of %d for %d inputs, %d groups in %d outputs)\n",
            classify_block_refusal_text(refusal), n_steps, ld, width, n_groups, e->sh.output_size);
    abort();
  }
  RecurNN *net = set->nets[0];
  const int n = set->n;
  const size_t stride = classify_mask_stride(n);
  if (e->sh.bI || net->presynaptic_noise != 0.0f || e->xchg_world || rnn_amd_dist_world() > 1) {
    u8 *trains = ramd_zalloc(stride);
    for (int t = 0; t < n_steps; t++) {
      classify_generation_host(set, features + (size_t)t * n * ld, ld, targets + (size_t)t * n * n_groups, n_groups,
                               group_offset, group_size, error_weight, learning_style, momentum_soft_start, condition, trains);
    }
    free(trains);
    return;
  }
  /* the block: features, then -- staged on the host as one piece -- targets, masks, gate words (zero), groups, weights */
  const size_t n_feat = (size_t)n_steps * n * ld, n_tg = (size_t)n_steps * n * n_groups;
  const size_t n_weights = error_weight ? (size_t)e->sh.output_size : 0;
  size_t bytes = 0;
  const size_t at_feat = automaton_room(&bytes, n_feat * sizeof(float));
  const size_t at_tg = automaton_room(&bytes, n_tg * sizeof(int));
  const size_t at_masks = automaton_room(&bytes, (size_t)n_steps * stride);
  const size_t at_gates = automaton_room(&bytes, (size_t)n_steps * sizeof(unsigned));
  const size_t at_groups = automaton_room(&bytes, (size_t)2 * n_groups * sizeof(int));
  const size_t at_weights = automaton_room(&bytes, n_weights * sizeof(float));
  ramd_engine_ensure_device(e);
  if (bytes > e->d_classify_bytes) {
    ramd_dsync(); /* (an earlier block's generations may still be reading the old one) */
    ramd_dev_free(e->d_classify);
    e->d_classify = ramd_dev_alloc(bytes);
    e->d_classify_bytes = bytes;
  }
  char *base = e->d_classify;
  char *tail = ramd_zalloc(bytes - at_tg); /* (zeroed: the gate words, the masks' padding) */
  u8 *masks = (u8 *)(tail + (at_masks - at_tg));
  int *active = ramd_zalloc((size_t)n_steps * sizeof(int));
  memcpy(tail, targets, n_tg * sizeof(int));
  classify_block_decisions(targets, n_steps, n, n_groups, group_size, masks, active, NULL);
  memcpy(tail + (at_groups - at_tg), group_offset, (size_t)n_groups * sizeof(int));
  memcpy(tail + (at_groups - at_tg) + (size_t)n_groups * sizeof(int), group_size, (size_t)n_groups * sizeof(int));
  if (error_weight) {
    memcpy(tail + (at_weights - at_tg), error_weight, n_weights * sizeof(float));
  }
  ramd_upload_q(base + at_feat, features, n_feat * sizeof(float));
  ramd_upload(base + at_tg, tail, bytes - at_tg);
  const float *d_feat = (const float *)(base + at_feat);
  const int *d_tg = (const int *)(base + at_tg);
  const int *d_goff = (const int *)(base + at_groups), *d_gsize = d_goff + n_groups;
  const float *d_weight = error_weight ? (const float *)(base + at_weights) : NULL;
  unsigned *d_gates = (unsigned *)(base + at_gates);
  int largest = 1;
  for (int i = 0; i < n_groups; i++) {
    largest = RAMD_MAX(largest, group_size[i]);
  }
  for (int t = 0; t < n_steps; t++) {
    rnn_bptt_clear_deltas(net); /* (lazy: the delta call simply does not accumulate) */
    const float *x = d_feat + (size_t)t * n * ld;
    const int *gt = d_tg + (size_t)t * n * n_groups;
    const u8 *mask = masks + (size_t)t * stride;
    /* generation t - 1's rnn_bptt_advance rides in this forward launch; the last one's follows the loop */
    const int advance = t > 0;
    /* the one-launch top where rnn_amd_set_opinion_grouped_softmax takes it: its output layer sums in another order than
     * the separate kernels', and the block keeps the bits of the loop of rnn_amd_classify_generation at every set size */
    if (dense_top_ok(set, x) && n % 4 == 0) {
      const RamdHandover left = set_forward(set, RAMD_IN_DENSE, x, ld, 0, NULL, advance, RAMD_FWD_FOR_DENSE_TOP);
      if (!ramd_launch_dense_top(ramd_stream, &e->sh, &e->b, set->row0, n, left, NULL, 0, 0, n_groups, d_goff, d_gsize, gt,
                                 d_weight, 0, d_gates + t)) {
        fprintf(stderr, "librecur_amd: rnn_amd_set_classify_steps: the top launch declined a shape it had accepted\n");
        abort();
      }
      set_streams_dev_wrote(set);
      ramd_top_done_set(e, set->row0, n, 1);
      if (!e->top_done_mask) {
        e->top_done_mask = ramd_zalloc((size_t)e->sh.Scap + 4);
      }
      memcpy(e->top_done_mask, mask, (size_t)n);
    } else {
      set_forward(set, RAMD_IN_DENSE, x, ld, 0, NULL, advance, RAMD_FWD_WHOLE);
      ramd_launch_grouped_softmax_error(ramd_stream, &e->sh, &e->b, set->row0, n, n_groups, largest, d_goff, d_gsize, gt,
                                        d_weight, d_gates + t);
      set_streams_dev_wrote(set);
    }
    if (active[t]) {
      /* never with the delta GEMM's update epilogue: the gate needs the optimiser launch of its own */
      set_calc_deltas_masked(set, 1, NULL, mask, (const u8 *)(base + at_masks) + (size_t)t * stride, 0, NULL, 0, NULL);
      ramd_apply_learning(net, learning_style,
                          rnn_calculate_momentum_soft_start(net->generation, net->bptt->momentum, momentum_soft_start), NULL,
                          d_gates + t);
    }
    if (condition) {
      rnn_condition_net(net);
    }
  }
  rnn_amd_set_advance(set);
  free(active);
  free(tail);
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
  check_text_pos(e, i, 0, "rnn_amd_set_char_step_fused");
  RecurNN *net = set->nets[0];
  const RamdShape *s = &e->sh;
  const int j = set->row0;
  const int batched = batch_size > 1;
  unsigned top_done = 0;
  if (ramd_text_top_ok(s)) { /* advance + hidden layer, then output layer, loss and top backprop in one launch */
    const RamdHandover left = set_forward(set, RAMD_IN_TEXT, NULL, 0, i, NULL, 1, RAMD_FWD_FOR_TEXT_TOP);
    ramd_launch_text_top(ramd_stream, s, &e->b, j, 1, left);
    top_done = RAMD_TOP_DONE;
  } else {
    set_forward(set, RAMD_IN_TEXT, NULL, 0, i, NULL, 1, RAMD_FWD_WHOLE); /* advance + one-hot opinion */
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
  set_streams_dev_wrote(set);
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
