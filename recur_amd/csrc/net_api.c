/* net_api.c -- the reference's RecurNN API for one net (recur-nn.h:269-334; behaviour of recur-nn.c and
 * recur-nn-init.c; gnu11 C) on top of engine.c and the HIP kernels in kernels_*.hip: construction, clones and training
 * sets, rnn_opinion, rnn_bptt_*, rnn_apply_learning with the one statement of the update rule, conditioning, logging,
 * a text through one net.  What the batched calls (set_api.c, set_loss.c, set_train.c) share with these lives here too. */
#define RAMD_HIP_HOST 1
#include "rnn_host.h"

/* ------------------------------------------------- construction (host only) -- */

static size_t round4(size_t x) { return (x + 3) & ~(size_t)3; }

/* rnn_bptt_advance (recur-nn.c:696-704), host side */
void ramd_host_advance(RecurNN *net) {
  RecurNNBPTT *bptt = net->bptt;
  bptt->index++;
  if (bptt->index == bptt->depth) {
    bptt->index -= bptt->depth;
  }
  net->input_layer = bptt->history + (size_t)bptt->index * net->i_size;
  net->real_inputs = net->input_layer + net->hidden_size + 1;
}

/* new_bptt (recur-nn-init.c:6-78): which arrays exist depends on the flags;
 * the order inside the block is ours. */
static RecurNNBPTT *bptt_new(RecurNN *net, int depth, float learn_rate, float momentum,
                             u32 flags) {
  RecurNNBPTT *bptt = ramd_zalloc(sizeof(RecurNNBPTT));
  int own_momentums = !(flags & RNN_NET_FLAG_NO_MOMENTUMS);
  int own_deltas = !(flags & RNN_NET_FLAG_NO_DELTAS);
  int aux_arrays = !!(flags & RNN_NET_FLAG_AUX_ARRAYS);
  size_t ih = (size_t)net->ih_size, ho = (size_t)net->ho_size;
  size_t I = net->i_size, O = net->o_size;
  size_t n = O + 2 * I + (size_t)depth * I;
  if (own_momentums) n += ih + ho;
  if (own_deltas) n += 2 * ih + ho;
  if (aux_arrays) n += ih + ho;
  float *fm = ramd_zalloc(n * sizeof(float));
  bptt->mem = fm;
  bptt->depth = depth;
  bptt->learn_rate = learn_rate;
  bptt->momentum = momentum;
  bptt->momentum_weight = RNN_MOMENTUM_WEIGHT;
#define TAKE(field, count) do { bptt->field = fm; fm += (count); } while (0)
  TAKE(o_error, O);
  TAKE(i_error, I);
  TAKE(h_error, I); /* i_size long so the two can be swapped, recur-nn-init.c:39-41 */
  TAKE(history, (size_t)depth * I);
  if (own_momentums) {
    TAKE(ih_momentum, ih);
    TAKE(ho_momentum, ho);
  }
  if (own_deltas) {
    TAKE(ih_delta, ih);
    TAKE(ho_delta, ho);
    TAKE(ih_delta_tmp, ih);
  }
  if (aux_arrays) {
    TAKE(ih_aux, ih);
    TAKE(ho_aux, ho);
  }
#undef TAKE
  bptt->index = 0;
  bptt->ho_scale = 1.0f;
  bptt->ih_scale = 1.0f;
  bptt->min_error_factor = BASE_MIN_ERROR_FACTOR * net->h_size;
  return bptt;
}

static RecurNN *net_new(uint input_size, uint hidden_size, uint output_size, u32 flags,
                        u64 rng_seed, const char *log_file, int bptt_depth, float learn_rate,
                        float momentum, float presynaptic_noise, rnn_activation activation,
                        RamdEngine *borrow) {
  RecurNN *net = ramd_zalloc(sizeof(RecurNN));
  /* padded sizes, recur-nn-init.c:87-91 */
  size_t i_size = round4((size_t)hidden_size + input_size + 1);
  size_t h_size = round4((size_t)hidden_size + 1);
  size_t o_size = round4(output_size);
  size_t ih_size = i_size * h_size, ho_size = h_size * o_size;
  net->i_size = (int)i_size;
  net->h_size = (int)h_size;
  net->o_size = (int)o_size;
  net->input_size = (int)input_size;
  net->hidden_size = (int)hidden_size;
  net->output_size = (int)output_size;
  net->ih_size = (int)ih_size;
  net->ho_size = (int)ho_size;
  net->generation = 0;
  net->flags = flags;
  net->presynaptic_noise = presynaptic_noise;
  if (activation >= RNN_ACTIVATION_LAST) {
    activation = RNN_RELU;
  }
  net->activation = activation;
  ramd_init_rand64_maybe_randomly(&net->rng, rng_seed);

  size_t n = RAMD_HDR_FLOATS + i_size + h_size + o_size;
  if (flags & RNN_NET_FLAG_OWN_WEIGHTS) {
    n += ih_size + ho_size;
  }
  float *fm = ramd_zalloc(n * sizeof(float));
  net->mem = fm;
  RamdPriv *priv = (RamdPriv *)fm;
  priv->magic = RAMD_MAGIC;
  priv->stream = priv->fwd = -1;
  priv->host_valid = 1;
  fm += RAMD_HDR_FLOATS;
  net->input_layer = fm; fm += i_size;
  net->hidden_layer = fm; fm += h_size;
  net->output_layer = fm; fm += o_size;
  if (flags & RNN_NET_FLAG_OWN_WEIGHTS) {
    net->ih_weights = fm; fm += ih_size;
    net->ho_weights = fm; fm += ho_size;
  }
  if (flags & RNN_NET_FLAG_OWN_BPTT) {
    net->bptt = bptt_new(net, bptt_depth, learn_rate, momentum, flags);
    ramd_host_advance(net); /* recur-nn-init.c:133: the first slot in use is 1 */
  } else {
    net->real_inputs = net->input_layer + net->hidden_size + 1;
  }
  if (flags & RNN_NET_FLAG_OWN_WEIGHTS) {
    ramd_engine_attach(ramd_engine_new(net), net);
  } else if (borrow) {
    ramd_engine_attach(borrow, net);
  }
  if (log_file) {
    rnn_set_log_file(net, log_file, flags & RNN_NET_FLAG_LOG_APPEND);
  }
  return net;
}

/* recur-nn.h:269-271 / recur-nn-init.c:80-143 */
RecurNN *rnn_new(uint input_size, uint hidden_size, uint output_size, u32 flags, u64 rng_seed,
                 const char *log_file, int bptt_depth, float learn_rate, float momentum,
                 float presynaptic_noise, rnn_activation activation) {
  return net_new(input_size, hidden_size, output_size, flags, rng_seed, log_file, bptt_depth,
                 learn_rate, momentum, presynaptic_noise, activation, NULL);
}

/* recur-nn-init.c:158-192.  Like the reference, nothing ever frees a layer: every
 * clone borrows the pointer (recur-nn-init.c:345-346). */
RecurExtraLayer *rnn_new_extra_layer(int input_size, int output_size, int overlap, u32 flags) {
  RecurExtraLayer *layer = ramd_zalloc(sizeof(RecurExtraLayer));
  layer->input_size = input_size;
  layer->output_size = output_size;
  layer->overlap = overlap;
  layer->learn_rate_scale = 1.0;
  layer->i_size = (int)round4(input_size + 1);
  layer->o_size = (int)round4(output_size);
  size_t m = (size_t)layer->i_size * layer->o_size;
  int aux = !!(flags & RNN_NET_FLAG_AUX_ARRAYS);
  size_t n = m * (3 + aux) + 2 * (size_t)(layer->i_size + layer->o_size);
  float *fm = ramd_zalloc(n * sizeof(float));
  layer->mem = fm;
  layer->momentums = fm; fm += m;
  layer->inputs = fm; fm += layer->i_size;
  layer->weights = fm; fm += m;
  layer->outputs = fm; fm += layer->o_size;
  layer->delta = fm; fm += m;
  layer->i_error = fm; fm += layer->i_size;
  layer->o_error = fm; fm += layer->o_size;
  if (aux) {
    layer->aux = fm;
  }
  return layer;
}

/* recur-nn-init.c:194-219 */
RecurNN *rnn_new_with_bottom_layer(int n_inputs, int r_input_size, int hidden_size,
                                   int output_size, u32 flags, u64 rng_seed,
                                   const char *log_file, int bptt_depth, float learn_rate,
                                   float momentum, float presynaptic_noise,
                                   rnn_activation activation, int convolutional_overlap) {
  if (r_input_size == 0) {
    flags &= ~RNN_NET_FLAG_BOTTOM_LAYER;
    return rnn_new(n_inputs, hidden_size, output_size, flags, rng_seed, log_file, bptt_depth,
                   learn_rate, momentum, presynaptic_noise, activation);
  }
  flags |= RNN_NET_FLAG_BOTTOM_LAYER;
  RecurNN *net = rnn_new(r_input_size, hidden_size, output_size, flags, rng_seed, log_file,
                         bptt_depth, learn_rate, momentum, presynaptic_noise, activation);
  net->bottom_layer = rnn_new_extra_layer(n_inputs, r_input_size, convolutional_overlap,
                                          net->flags);
  return net;
}

/* recur-nn-init.c:145-155 */
void rnn_delete_net(RecurNN *net) {
  RamdPriv *p = ramd_priv(net);
  RamdEngine *e = p->eng;
  if (e) {
    if (e->owner == net) {
      ramd_engine_delete(e);
    } else {
      /* the row stays reserved; forget the pointer */
      if (p->stream >= 0 && p->stream < e->n_streams) e->streams[p->stream] = e->owner;
      if (p->fwd >= 0 && p->fwd < e->n_fwd) e->fwd[p->fwd] = e->owner;
      /* trailing rows can be given back */
      while (e->n_streams > 0 && e->streams[e->n_streams - 1] == e->owner &&
             ramd_priv(e->owner)->stream != e->n_streams - 1) {
        e->n_streams--;
      }
      while (e->n_fwd > 0 && e->fwd[e->n_fwd - 1] == e->owner &&
             ramd_priv(e->owner)->fwd != e->n_fwd - 1) {
        e->n_fwd--;
      }
    }
  }
  if (net->bptt && (net->flags & RNN_NET_FLAG_OWN_BPTT)) {
    free(net->bptt->mem);
    free(net->bptt);
  }
  if (net->log) {
    fclose(net->log);
  }
  free(net->mem);
  free(net);
}

/* recur-nn-init.c:268-283 */
void rnn_set_log_file(RecurNN *net, const char *log_file, int append_dont_truncate) {
  if (net->log) {
    fclose(net->log);
  }
  if (log_file) {
    net->log = fopen(log_file, append_dont_truncate ? "a" : "w");
    if (!append_dont_truncate) {
      rnn_log_int(net, "generation", net->generation);
    }
  } else {
    net->log = NULL;
  }
}

/* recur-nn-init.c:296-350 */
RecurNN *rnn_clone(RecurNN *parent, u32 flags, u64 rng_seed, const char *log_file) {
  if (rng_seed == RECUR_RNG_SUBSEED) {
    if (ramd_priv(parent)->eng && !ramd_priv(parent)->host_valid) {
      ramd_need_host(parent, RNN_AMD_STREAM);
    }
    ramd_priv(parent)->dev_valid = 0;
    do {
      rng_seed = ramd_rand64(&parent->rng);
    } while (rng_seed == RECUR_RNG_RANDOM_SEED);
  }
  float learn_rate = 0, momentum = 0;
  int bptt_depth = 0;
  if (parent->bptt && (flags & RNN_NET_FLAG_OWN_BPTT)) {
    learn_rate = parent->bptt->learn_rate;
    bptt_depth = parent->bptt->depth;
    momentum = parent->bptt->momentum;
  }
  if (!(parent->bptt && (flags & RNN_NET_FLAG_OWN_BPTT))) {
    flags &= ~RNN_NET_FLAG_OWN_BPTT; /* no parent bptt to model it on */
  }
  RamdEngine *pe = ramd_engine_of(parent);
  RecurNN *net = net_new(parent->input_size, parent->hidden_size, parent->output_size, flags,
                         rng_seed, log_file, bptt_depth, learn_rate, momentum,
                         parent->presynaptic_noise, parent->activation,
                         (flags & RNN_NET_FLAG_OWN_WEIGHTS) ? NULL : pe);
  if (net->bptt) {
    net->bptt->momentum_weight = parent->bptt->momentum_weight;
    if (flags & RNN_NET_FLAG_NO_MOMENTUMS) {
      net->bptt->ih_momentum = parent->bptt->ih_momentum;
      net->bptt->ho_momentum = parent->bptt->ho_momentum;
    }
    if (flags & RNN_NET_FLAG_NO_DELTAS) {
      net->bptt->ih_delta = parent->bptt->ih_delta;
      net->bptt->ho_delta = parent->bptt->ho_delta;
    }
  }
  if (flags & RNN_NET_FLAG_OWN_WEIGHTS) {
    ramd_need_host(parent, RNN_AMD_WEIGHTS);
    memcpy(net->ih_weights, parent->ih_weights, (size_t)net->ih_size * sizeof(float));
    memcpy(net->ho_weights, parent->ho_weights, (size_t)net->ho_size * sizeof(float));
  } else {
    net->ih_weights = parent->ih_weights;
    net->ho_weights = parent->ho_weights;
  }
  net->bottom_layer = parent->bottom_layer;
  net->generation = parent->generation;
  net->presynaptic_noise = parent->presynaptic_noise;
  return net;
}

/* recur-nn-init.c:221-243 */
RecurNN **rnn_new_training_set(RecurNN *prototype, int n_nets) {
  if (n_nets < 1) {
    fprintf(stderr, "A training set of size %d is not possible\n", n_nets);
    return NULL;
  }
  RecurNN **nets = ramd_zalloc(n_nets * sizeof(RecurNN *));
  nets[0] = prototype;
  u32 flags = prototype->flags;
  flags &= ~RNN_NET_FLAG_OWN_WEIGHTS;
  flags |= RNN_NET_FLAG_NO_MOMENTUMS;
  flags |= RNN_NET_FLAG_NO_DELTAS;
  for (int i = 1; i < n_nets; i++) {
    nets[i] = rnn_clone(prototype, flags, RECUR_RNG_SUBSEED, NULL);
    nets[i]->bptt->ih_delta = prototype->bptt->ih_delta;
    nets[i]->bptt->ih_delta_tmp = prototype->bptt->ih_delta_tmp;
    nets[i]->bptt->ho_delta = prototype->bptt->ho_delta;
  }
  return nets;
}

/* One shard of a training set whose streams are spread over several processes (one per
 * GPU).  The reference seeds clone g from the g-th draw of the prototype's generator
 * (recur-nn-init.c:232-241, 300-305); every rank replays ALL the draws so that global
 * stream g gets the reference's generator wherever it lives, and keeps its own range. */
RecurNN **rnn_amd_new_training_set_shard(RecurNN *prototype, int n_local, int global_first,
                                         int global_count) {
  if (n_local < 1 || global_first < 0 || global_first + n_local > global_count) {
    fprintf(stderr, "A training set shard of %d streams at %d of %d is not possible\n", n_local,
            global_first, global_count);
    return NULL;
  }
  RecurNN **nets = ramd_zalloc(n_local * sizeof(RecurNN *));
  nets[0] = prototype;
  u32 flags = prototype->flags;
  flags &= ~RNN_NET_FLAG_OWN_WEIGHTS;
  flags |= RNN_NET_FLAG_NO_MOMENTUMS;
  flags |= RNN_NET_FLAG_NO_DELTAS;
  if (ramd_priv(prototype)->eng && !ramd_priv(prototype)->host_valid) {
    ramd_need_host(prototype, RNN_AMD_STREAM);
  }
  ramd_priv(prototype)->dev_valid = 0;
  u64 first_seed = 0;
  for (int g = 1; g < global_count; g++) {
    u64 seed;
    do {
      seed = ramd_rand64(&prototype->rng);
    } while (seed == RECUR_RNG_RANDOM_SEED);
    int j = g - global_first;
    if (j == 0) {
      first_seed = seed;
    } else if (j > 0 && j < n_local) {
      nets[j] = rnn_clone(prototype, flags, seed, NULL);
      nets[j]->bptt->ih_delta = prototype->bptt->ih_delta;
      nets[j]->bptt->ih_delta_tmp = prototype->bptt->ih_delta_tmp;
      nets[j]->bptt->ho_delta = prototype->bptt->ho_delta;
    }
  }
  if (global_first > 0) {
    /* this rank's first stream is global stream global_first: its generator, not the
     * prototype's (which belongs to global stream 0 on rank 0; see ramd_shared_rng) */
    ramd_init_rand64_maybe_randomly(&prototype->rng, first_seed);
  }
  if (ramd_priv(prototype)->eng && n_local != global_count) {
    ramd_priv(prototype)->eng->sharded_sticky = 1;
    ramd_priv(prototype)->eng->sharded = 1;
  }
  return nets;
}

/* recur-nn-init.c:245-257 */
void rnn_delete_training_set(RecurNN **nets, int n_nets, int leave_prototype) {
  /* clones first: the prototype owns the weights and the device image */
  for (int i = n_nets - 1; i >= 1; i--) {
    if (nets[i]) {
      rnn_delete_net(nets[i]);
    }
  }
  if (!leave_prototype && nets[0]) {
    rnn_delete_net(nets[0]);
  }
  free(nets);
}

/* ------------------------------------------------------------ scalars push -- */

/* learn_rate is host-authoritative (callers write bptt->learn_rate, e.g.
 * charmodel-predict.c:107, and clones keep their stale copy: SURVEY quirk 4). */
void ramd_push_learn_rates(RamdEngine *e, int row0, int nrows) {
  int dirty = 0;
  for (int j = row0; j < row0 + nrows; j++) {
    float lr = e->streams[j]->bptt->learn_rate;
    if (lr != e->lr_pushed[j]) {
      e->lr_pushed[j] = lr;
      dirty = 1;
    }
  }
  if (dirty) {
    ramd_mail_in(e->b.lr + row0, e->lr_pushed + row0, nrows * sizeof(float)); /* leaves with the next flush */
  }
}

/* The ring indices are host-authoritative too: rnn_bptt_advance only steps the host's copy,
 * and the device's is brought up to date here, before the next launch that reads it (the set
 * calls that advance on the device record the new value in the mirror themselves). */
void ramd_push_indices(RamdEngine *e, int row0, int nrows) {
  int dirty = 0;
  for (int j = row0; j < row0 + nrows && j < e->n_streams; j++) {
    int idx = e->streams[j]->bptt->index;
    if (idx != e->idx_pushed[j]) {
      e->idx_pushed[j] = idx;
      dirty = 1;
    }
  }
  if (dirty) {
    ramd_mail_in(e->b.idx + row0, e->idx_pushed + row0, nrows * sizeof(int));
  }
}

/* device mef / ih_scale -> host structs, for a range of streams */
void ramd_pull_scalars(RamdEngine *e, int row0, int nrows) {
  float *tmp = malloc(2 * nrows * sizeof(float));
  ramd_d2h(tmp, e->b.mef + row0, nrows * sizeof(float));
  ramd_d2h(tmp + nrows, e->b.ih_scale + row0, nrows * sizeof(float));
  ramd_dsync();
  for (int j = 0; j < nrows; j++) {
    RecurNNBPTT *bp = e->streams[row0 + j]->bptt;
    bp->min_error_factor = tmp[j];
    bp->ih_scale = tmp[nrows + j];
  }
  free(tmp);
}

/* The ring position every stream of [row0, row0 + nrows) shares, or -1.  The
 * host mirrors the indices exactly (they only ever change by rnn_bptt_advance). */
void ramd_set_uniform_idx(RamdEngine *e, int row0, int nrows) {
  int u = -1;
  if (e->dev_ready && row0 < e->n_streams && nrows > 0) {
    ramd_push_indices(e, row0, nrows);
  }
  if (row0 < e->n_streams && nrows > 0) {
    u = e->streams[row0]->bptt->index;
    for (int j = row0 + 1; j < row0 + nrows && j < e->n_streams; j++) {
      if (e->streams[j]->bptt->index != u) {
        u = -1;
        break;
      }
    }
  }
  e->b.uniform_idx = u;
  ramd_mail_in_flush(); /* whatever the caller queued for the launches that follow */
}

/* ----------------------------------------------------------------- logging -- */

/* What bptt_and_accumulate_error and rnn_bptt_calc_deltas write to net->log
 * (recur-nn.c:415-448, 766-771), rebuilt from the device's per-stream results. */
void ramd_log_bptt(RamdEngine *e, RecurNN *net, float mef_before) {
  if (!net->log) {
    return;
  }
  RamdPriv *p = ramd_priv(net);
  int j = p->stream, D = e->sh.D, S = e->sh.Scap;
  float top_raw, top_scaled, bptt_err, scale, mef;
  int depth, n_exec;
  float *es = malloc(D * sizeof(float));
  ramd_d2h(&top_raw, e->b.top_raw + j, 4);
  ramd_d2h(&top_scaled, e->b.top_scaled + j, 4);
  ramd_d2h(&bptt_err, e->b.bptt_err + j, 4);
  ramd_d2h(&scale, e->b.ih_scale + j, 4);
  ramd_d2h(&mef, e->b.mef + j, 4);
  ramd_d2h(&depth, e->b.depth_log + j, 4);
  ramd_d2h(&n_exec, e->b.n_exec + j, 4);
  HIP_OK(hipMemcpy2DAsync(es, sizeof(float), e->b.esum + j, S * sizeof(float), sizeof(float), D,
                          hipMemcpyDeviceToHost, ramd_stream));
  ramd_d2h(net->hidden_layer, e->b.hidden + (size_t)j * e->sh.H, e->sh.H * sizeof(float));
  ramd_dsync();
  float cum_error = 0.0f;
  for (int k = 0; k < n_exec; k++) {
    cum_error += sqrtf(es[k]);
  }
  free(es);
  float min_gain = MIN_ERROR_GAIN * top_scaled;
  float thr = RAMD_MIN(mef_before / net->bptt->learn_rate, min_gain);
  rnn_log_int(net, "depth", depth);
  rnn_log_float(net, "scaled_error", scale * bptt_err);
  rnn_log_float(net, "ih_scale", scale);
  rnn_log_float(net, "min_error_threshold", thr);
  rnn_log_float(net, "min_error_factor", mef);
  rnn_log_float(net, "cum_error", cum_error);
  if (net->flags & RNN_NET_FLAG_LOG_HIDDEN_SUM) {
    float hidden_sum = 0, hidden_magnitude = 0;
    int hidden_zeros = 0;
    for (int i = 0; i < net->h_size; i++) {
      float h = net->hidden_layer[i];
      hidden_sum += h;
      hidden_magnitude += h * h;
      hidden_zeros += (h == 0.0f);
    }
    rnn_log_float(net, "hidden_sum", hidden_sum);
    rnn_log_float(net, "hidden_magnitude", sqrtf(hidden_magnitude));
    rnn_log_float(net, "hidden_zeros", hidden_zeros / (float)net->hidden_size);
  }
  if (net->flags & RNN_NET_FLAG_LOG_WEIGHT_SUM) {
    ramd_engine_need_host(e, RNN_AMD_WEIGHTS);
    float weight_sum = 0.0f;
    for (int i = 0; i < net->ih_size; i++) {
      weight_sum += fabsf(net->ih_weights[i]);
    }
    rnn_log_float(net, "weight_sum", weight_sum);
  }
  rnn_log_float(net, "error_gain", bptt_err / (top_scaled + 1e-6));
  rnn_log_float(net, "top_error_scaled", top_scaled);
  rnn_log_float(net, "top_error_raw", top_raw);
}

/* ---------------------------------------------------------- per-net hot path -- */

/* recur-nn.h:310 */
void rnn_bptt_advance(RecurNN *net) {
  ramd_host_advance(net); /* the device's copy follows before the next launch that reads it: ramd_push_indices */
}

/* recur-nn.h:302 / recur-nn.c:83-154 for one stream */
float *rnn_opinion(RecurNN *net, const float *inputs, float presynaptic_noise) {
  RamdEngine *e = ramd_engine_of(net);
  RamdPriv *p = ramd_priv(net);
  ramd_engine_ensure_device(e);
  ramd_top_done_clear(e);
  ramd_engine_need_dev(e, RNN_AMD_WEIGHTS);
  const RamdShape *s = &e->sh;
  RecurExtraLayer *bl = s->bI ? net->bottom_layer : NULL;
  /* the caller's real inputs are authoritative: keep them across a refresh */
  float *keep = malloc(sizeof(float) * s->input_size);
  memcpy(keep, (inputs && !bl) ? inputs : net->real_inputs, sizeof(float) * s->input_size);
  ramd_stream_need_host(e, net);
  ramd_stream_need_dev(e, net);
  memcpy(net->real_inputs, keep, sizeof(float) * s->input_size);
  free(keep);
  int r = ramd_state_row(e, p);
  float *d_slot;
  /* everything that goes in travels in one mailbox launch, everything that comes back in
   * another, and the call ends with one synchronisation */
  if (p->stream >= 0) {
    d_slot = e->b.arena + ((size_t)net->bptt->index * s->Scap + p->stream) * s->I;
  } else {
    d_slot = e->b.arena + ((size_t)s->D * s->Scap + p->fwd) * s->I;
  }
  if (presynaptic_noise != 0.0f) { /* the host generator is the one the caller may have used */
    ramd_mail_in((char *)e->b.rng + (size_t)r * sizeof(rand_ctx), &net->rng, sizeof(rand_ctx));
    ramd_rng_written_from_host(e);
  }
  if (bl) { /* recur-nn.c:88-103: the layer's one input buffer is shared by every clone */
    bl->inputs[0] = 1.0f;
    if (inputs) {
      memcpy(bl->inputs + 1, inputs, sizeof(float) * bl->input_size);
    }
    ramd_mail_in(e->b.binp + (size_t)r * s->bI, bl->inputs, sizeof(float) * s->bI);
  } else {
    ramd_mail_in(d_slot + s->hidden_size + 1, net->real_inputs, sizeof(float) * s->input_size);
  }
  ramd_set_uniform_idx(e, p->stream >= 0 ? p->stream : e->n_streams, p->stream >= 0 ? 1 : 0);
  ramd_mail_in_flush();
  /* (the inputs are in place: the bottom layer's in its own row, the net's in the slot) */
  const RamdFwdCall call = {.row0 = r, .nrows = 1, .mode = RAMD_IN_KEEP, .global_count = 1, .noise = presynaptic_noise,
                            .one_net = 1};
  ramd_launch_forward(ramd_stream, s, &e->b, &call, NULL, NULL);
  if (bl) {
    ramd_mail_out(bl->outputs, e->b.bout + (size_t)r * s->bO, sizeof(float) * s->bO);
  }
  if (presynaptic_noise != 0.0f) {
    ramd_mail_out(&net->rng, (char *)e->b.rng + (size_t)r * sizeof(rand_ctx), sizeof(rand_ctx));
  }
  ramd_mail_out(net->input_layer, d_slot, sizeof(float) * s->I);
  ramd_mail_out(net->hidden_layer, e->b.hidden + (size_t)r * s->H, sizeof(float) * s->H);
  ramd_mail_out(net->output_layer, e->b.out + (size_t)r * s->O, sizeof(float) * s->O);
  ramd_mail_out_flush();
  return net->output_layer;
}

const int *ramd_push_ranges(RamdEngine *e, RecurErrorRange *ranges) {
  if (!ranges) {
    return NULL;
  }
  int n = 0;
  while (ranges[n].start >= 0) {
    n++;
  }
  if (n > 64) {
    fprintf(stderr, "librecur_amd: more than 64 error ranges\n");
    abort();
  }
  ramd_mail_in(e->d_ranges, ranges, (n + 1) * sizeof(RecurErrorRange));
  return e->d_ranges;
}

static void calc_deltas_one(RecurNN *net, int accumulate, RecurErrorRange *ranges, unsigned fused) {
  RamdEngine *e = ramd_engine_of(net);
  RamdPriv *p = ramd_priv(net);
  if (p->stream < 0) {
    fprintf(stderr, "librecur_amd: rnn_bptt_calc_deltas on a net without bptt\n");
    abort();
  }
  ramd_engine_ensure_device(e);
  ramd_top_done_clear(e); /* (a per-net call between a set's one-call loss and its delta call: that set's top backprop is redone) */
  const RamdShape *s = &e->sh;
  int j = p->stream;
  if (fused) {
    /* rnn_bptt_calculate never writes ho_delta: after rnn_bptt_clear_deltas the reference has
     * zeros there (recur-nn.c:681-693), so the pending clear is carried out, not dropped */
    ramd_deltas_materialize(e);
  }
  if (e->deltas_zero_pending) { /* the sum into zeros is the sum */
    accumulate = 0;
    e->deltas_zero_pending = 0;
  }
  ramd_engine_need_dev(e, RNN_AMD_WEIGHTS | (accumulate ? RNN_AMD_DELTAS : 0));
  e->kept_live = 0; /* (a set call's kept sums: added up just now if this call accumulates, otherwise overwritten) */
  if (fused) {
    /* (the fused path rewrites ih_delta only: the rest of the delta arrays has to be the device's
     * own before they are declared written -- after a regrow the device copy is blank) */
    ramd_engine_need_dev(e, RNN_AMD_MOMENTUMS | RNN_AMD_DELTAS);
  }
  float *keep = malloc(sizeof(float) * s->O);
  memcpy(keep, net->bptt->o_error, sizeof(float) * s->O);
  ramd_stream_need_host(e, net);
  ramd_stream_need_dev(e, net);
  memcpy(net->bptt->o_error, keep, sizeof(float) * s->O);
  free(keep);
  RecurNNBPTT *bp = net->bptt;
  float mef_before = bp->min_error_factor;
  ramd_mail_in(e->b.o_error + (size_t)j * s->O, bp->o_error, sizeof(float) * s->O);
  ramd_mail_in(e->b.mef + j, &bp->min_error_factor, sizeof(float));
  if (ranges) {
    /* the sparse top path reads last time's h_error */
    ramd_err_flush(e);
    ramd_mail_in(e->b.err_a + (size_t)j * s->I, bp->h_error, sizeof(float) * s->I);
  }
  ramd_push_learn_rates(e, j, 1);
  const int *d_ranges = ramd_push_ranges(e, ranges);
  if (e->err_pending) {
    ramd_err_flush(e);
  }
  ramd_set_uniform_idx(e, j, 1);
  ramd_mail_in_flush();
  ramd_launch_calc_deltas(ramd_stream, s, &e->b, j, 1, accumulate, d_ranges, 0, NULL,
                          net->flags | (fused ? RAMD_NO_HO_DELTA : 0) | (fused == 2 ? RAMD_IH_SCALE_IN_RATE : 0), NULL);
  if (s->bI && !fused) { /* the fused path passes no bottom error (recur-nn.c:972, 986) */
    if (accumulate) {
      ramd_engine_need_dev(e, RNN_AMD_DELTAS);
    }
    ramd_launch_bottom_deltas(ramd_stream, s, &e->b, j, 1, accumulate, NULL);
    ramd_mail_out(net->bottom_layer->o_error, e->b.bcarry + (size_t)e->b.bcarry_cur * s->bO,
             sizeof(float) * s->bO);
  }
  ramd_engine_dev_wrote(e, RNN_AMD_DELTAS);
  ramd_err_after_calc(e, j, 1);
  ramd_err_flush(e); /* (the images go back with this call) */
  ramd_mail_out(bp->h_error, e->b.err_a + (size_t)j * s->I, sizeof(float) * s->I);
  ramd_mail_out(bp->i_error, e->b.err_b + (size_t)j * s->I, sizeof(float) * s->I);
  ramd_mail_out(&bp->min_error_factor, e->b.mef + j, sizeof(float));
  ramd_mail_out(&bp->ih_scale, e->b.ih_scale + j, sizeof(float));
  ramd_mail_out_flush();
  net->generation++;
  ramd_log_bptt(e, net, mef_before);
}

/* recur-nn.h:316 / recur-nn.c:707-772 */
void rnn_bptt_calc_deltas(RecurNN *net, int accumulate_delta, RecurErrorRange *top_error_ranges) {
  calc_deltas_one(net, accumulate_delta, top_error_ranges, 0);
  rnn_log_int(net, "generation", net->generation);
}

/* recur-nn.h:309 / recur-nn.c:681-693 */
void rnn_bptt_clear_deltas(RecurNN *net) {
  RamdEngine *e = ramd_engine_of(net);
  ramd_engine_ensure_device(e);
  e->kept_live = 0; /* sums nobody asked for */
  if (e->sh.bI) { /* the bottom layer's error accumulator is cleared with them: at once */
    e->deltas_zero_pending = 0;
    ramd_launch_clear_deltas(ramd_stream, &e->sh, &e->b);
  } else {
    e->deltas_zero_pending = 1; /* see ramd_deltas_materialize */
  }
  ramd_engine_dev_wrote(e, RNN_AMD_DELTAS);
}

/* recur-nn.h:313 / recur-nn.c:595-599 */
float rnn_calculate_momentum_soft_start(float generation, float max_momentum, float x) {
  return RAMD_MIN(max_momentum, 1.0f - x / (1.0f + generation + 2.0f * x));
}

void ramd_check_method_arrays(RamdEngine *e, int method) {
  if ((method == RNN_ADADELTA || method == RNN_RPROP) && !e->has_aux) {
    fprintf(stderr, "librecur_amd: learning method %d needs RNN_NET_FLAG_AUX_ARRAYS\n", method);
    abort();
  }
}

/* rnn_apply_learning's arrays in one launch: top layer, recurrent layer and, when there
 * is one, the bottom layer with its own rate scale (recur-nn.c:606-676; the arrays are
 * disjoint, so the reference's order between them does not matter) */
static void apply_all(RamdEngine *e, int method, float lr, float lr_top, float momentum,
                      float mw, const RamdPendingDelta *pend, const unsigned *gate) {
  RamdBuffers *b = &e->b;
  ramd_check_method_arrays(e, method);
  float *w[3] = {b->ho_w, b->ih_w, b->bw};
  const float *d[3] = {b->ho_delta, b->ih_delta, b->bdelta};
  float *m[3] = {b->ho_m, b->ih_m, b->bm};
  float *aux[3] = {b->ho_aux, b->ih_aux, b->baux};
  size_t n[3] = {e->ho_size, e->ih_size, (size_t)e->sh.bI * e->sh.bO};
  float rate[3] = {lr_top, lr,
                   e->sh.bI ? lr * e->owner->bottom_layer->learn_rate_scale : 0.0f};
  ramd_launch_apply_multi(ramd_stream, method, e->sh.bI ? 3 : 2, w, d, m, aux, n, rate, momentum, mw,
                          NULL, pend, gate);
}

/* The update rule, stated once (recur-nn.c:601-678), for rnn_apply_learning, the update fused into the delta GEMM
 * (set_step) and the exchange's sharded update: returns the kernel's method -- the momentum styles but NESTEROV, and
 * styles out of range, are the weighted rule with their own momentum weight -- and leaves that weight and the rates. */
int ramd_update_rule(const RecurNNBPTT *bptt, int learning_style, float momentum, float *mw, float *rate, float *ho_rate) {
  if (learning_style == RNN_MOMENTUM_SIMPLIFIED_NESTEROV) {
    *mw = momentum / (1.0 + momentum);
  } else if (learning_style == RNN_MOMENTUM_CLASSICAL) {
    *mw = 1.0f;
  } else {
    *mw = bptt->momentum_weight;
  }
  *rate = bptt->learn_rate;
  *ho_rate = bptt->learn_rate * bptt->ho_scale;
  if (learning_style == RNN_MOMENTUM_SIMPLIFIED_NESTEROV || learning_style == RNN_MOMENTUM_CLASSICAL ||
      learning_style >= RNN_LAST_LEARNING_METHOD || learning_style < 0) {
    return RNN_MOMENTUM_WEIGHTED;
  }
  return learning_style;
}

/* recur-nn.h:312 / recur-nn.c:601-678.  gate (or NULL): a device word that switches the update off where it is 0
 * (ramd_launch_apply_multi); the delta sums are formed and stored either way */
void ramd_apply_learning(RecurNN *net, int learning_method, float momentum,
                           const RamdPendingDelta *pend, const unsigned *gate) {
  RamdEngine *e = ramd_engine_of(net);
  ramd_engine_ensure_device(e);
  if (!pend && e->kept_live && e->dev_ready) {
    /* the last set call's sums, still planes: this launch adds them up (and stores them) on its way */
    pend = &e->kept;
    e->kept_live = 0;
    ramd_engine_need_dev(e, RNN_AMD_WEIGHTS | RNN_AMD_MOMENTUMS);
  } else {
    ramd_engine_need_dev(e, RNN_AMD_WEIGHTS | RNN_AMD_MOMENTUMS | RNN_AMD_DELTAS);
  }
  float mw, rate, ho_rate;
  const int kernel_method = ramd_update_rule(net->bptt, learning_method, momentum, &mw, &rate, &ho_rate);
  apply_all(e, kernel_method, rate, ho_rate, momentum, mw, pend, gate);
  ramd_engine_dev_wrote(e, RNN_AMD_WEIGHTS | RNN_AMD_MOMENTUMS);
}

void rnn_apply_learning(RecurNN *net, int learning_method, float momentum) {
  ramd_apply_learning(net, learning_method, momentum, NULL, NULL);
}

/* recur-nn.h:319 / recur-nn.c:782-855 */
void rnn_condition_net(RecurNN *net) {
  u32 mask = net->flags >> RNN_COND_USE_OFFSET;
  u32 m = net->generation % RNN_CONDITIONING_INTERVAL;
  if (((1u << m) & mask) == 0) {
    return;
  }
  RamdEngine *e = ramd_engine_of(net);
  ramd_engine_ensure_device(e);
  RamdBuffers *b = &e->b;
  switch (m) {
  case RNN_COND_BIT_SCALE:
    ramd_engine_need_dev(e, RNN_AMD_WEIGHTS);
    ramd_launch_scale(ramd_stream, b->ih_w, e->ih_size, WEIGHT_SCALE);
    ramd_launch_scale(ramd_stream, b->ho_w, e->ho_size, WEIGHT_SCALE);
    ramd_engine_dev_wrote(e, RNN_AMD_WEIGHTS);
    break;
  case RNN_COND_BIT_ZERO:
    ramd_engine_need_dev(e, RNN_AMD_WEIGHTS | RNN_AMD_MOMENTUMS);
    ramd_launch_zero_small(ramd_stream, b->ih_w, e->ih_size);
    ramd_launch_zero_small(ramd_stream, b->ho_w, e->ho_size);
    if (net->bptt) {
      ramd_launch_zero_small(ramd_stream, b->ih_m, e->ih_size);
      ramd_launch_zero_small(ramd_stream, b->ho_m, e->ho_size);
    }
    ramd_engine_dev_wrote(e, RNN_AMD_WEIGHTS | RNN_AMD_MOMENTUMS);
    break;
  case RNN_COND_BIT_RAND: {
    ramd_stream_need_host(e, net); /* the generator may have advanced on the device (noise) */
    rand_ctx tmp, *rng = ramd_shared_rng(net, &tmp); /* every replica takes the same damage */
    int t = ramd_rand_small_int(rng, net->ih_size + net->ho_size);
    float damage = (ramd_cheap_gaussian_noise(rng) * RANDOM_DAMAGE_FACTOR * net->h_size *
                    net->bptt->learn_rate);
    ramd_priv(net)->dev_valid = 0; /* and now it advanced on the host */
    ramd_engine_need_dev(e, RNN_AMD_WEIGHTS);
    if (t >= net->ih_size) {
      t -= net->ih_size;
      if (t % net->o_size < net->output_size) {
        ramd_launch_add_at(ramd_stream, b->ho_w, t, damage);
      }
    } else {
      int col = t % net->h_size;
      if (col >= 1 && col < net->hidden_size + 1) {
        ramd_launch_add_at(ramd_stream, b->ih_w, t, damage);
      }
    }
    ramd_engine_dev_wrote(e, RNN_AMD_WEIGHTS);
  } break;
  case RNN_COND_BIT_TALL_POPPY:
    ramd_engine_need_dev(e, RNN_AMD_WEIGHTS);
    ramd_launch_tall_poppy(ramd_stream, b->ih_w, e->ih_size, RNN_TALL_POPPY_THRESHOLD,
                           RNN_TALL_POPPY_SCALE, e->d_scratch);
    ramd_engine_dev_wrote(e, RNN_AMD_WEIGHTS);
    break;
  case RNN_COND_BIT_LAWN_MOWER:
    ramd_engine_need_dev(e, RNN_AMD_WEIGHTS);
    ramd_launch_clamp(ramd_stream, b->ih_w, e->ih_size, -RNN_LAWN_MOWER_THRESHOLD,
                      RNN_LAWN_MOWER_THRESHOLD);
    ramd_engine_dev_wrote(e, RNN_AMD_WEIGHTS);
    break;
  }
}

/* What follows the delta launch (flag RAMD_NO_HO_DELTA) of the single-net path that updates the weights at once, for
 * rnn_bptt_calculate and rnn_amd_set_char_step_fused: net->generation has been incremented already; the reference
 * tests the value before its increment (recur-nn.c:991, 1010). */
void ramd_fused_net_update(RamdEngine *e, RecurNN *net, int row, unsigned batch_size) {
  const RecurNNBPTT *bptt = net->bptt;
  const int batched = batch_size > 1;
  const int due = !batched || ((net->generation - 1) % batch_size) == 0;
  /* the top layer's immediate update and, when due, the recurrent layer's: one launch */
  ramd_launch_fused_updates(ramd_stream, &e->sh, &e->b, row, bptt->learn_rate, bptt->momentum, bptt->momentum_weight, due,
                            batched ? NULL : e->b.ih_scale + row);
  if (due && batched) { /* ih_delta only (recur-nn.c:991): ho_delta is not this path's */
    HIP_OK(hipMemsetAsync(e->b.ih_delta, 0, e->ih_size * sizeof(float), ramd_stream));
  }
  ramd_engine_dev_wrote(e, RNN_AMD_WEIGHTS | RNN_AMD_MOMENTUMS | RNN_AMD_DELTAS);
  rnn_condition_net(net);
}

/* recur-nn.h:311 / recur-nn.c:919-1019: the single-net path that updates the
 * weights at once.  Top layer: backprop with the old weights, then the
 * rank-1 update with momentum (no ho_scale, recur-nn.c:927); recurrent layer:
 * BPTT deltas (the per-stream ih_scale is already folded into them) applied
 * with the weighted-momentum rule, every step or every batch_size steps. */
void rnn_bptt_calculate(RecurNN *net, uint batch_size) {
  int batched = batch_size > 1;
  /* without batching the reference leaves the unscaled sum in ih_delta and multiplies the rate by
   * ih_scale (recur-nn.c:966-975); batched, ih_scale goes into the sum (977-994) */
  calc_deltas_one(net, batched, NULL, batched ? 1 : 2); /* also does generation++ */
  if (net->log) {
    rnn_log_int(net, "generation", net->generation);
  }
  ramd_fused_net_update(ramd_engine_of(net), net, ramd_priv(net)->stream, batch_size);
}

/* recur-nn.h:322 / recur-nn.c:8-16 */
void rnn_forget_history(RecurNN *net, int bptt_too) {
  RamdEngine *e = ramd_engine_of(net);
  ramd_stream_need_host(e, net);
  memset(net->hidden_layer, 0, net->h_size * sizeof(float));
  memset(net->input_layer, 0, (net->hidden_size + 1) * sizeof(float));
  if (bptt_too && net->bptt) {
    memset(net->bptt->history, 0, (size_t)net->bptt->depth * net->i_size * sizeof(float));
  }
  ramd_priv(net)->dev_valid = 0;
}

/* recur-nn.h:320 / recur-nn.c:887-904 */
void rnn_log_net(RecurNN *net) {
  if (net->log == NULL) {
    return;
  }
  if (net->bptt) {
    ramd_need_host(net, RNN_AMD_STREAM);
    float top_error = 0, hidden_error = 0;
    for (int i = 0; i < net->o_size; i++) {
      top_error += fabsf(net->bptt->o_error[i]);
    }
    for (int i = 0; i < net->h_size; i++) {
      hidden_error += fabsf(net->bptt->h_error[i]);
    }
    rnn_log_float(net, "output_error", top_error);
    rnn_log_float(net, "hidden_error", hidden_error);
  }
}

/* ------------------------------------------------ text through one net -- */

/* Runs one net over an encoded text without leaving the device: for every i < len - 1
 * a one_hot_opinion of text[i] (charmodel-helpers.h:16-33) and, from i = skip on, the
 * log2 probability the softmax gives text[i + 1].  With alphabet_len == 0 the softmax is
 * over the whole output row and sums[0] gets the sum of the logs (get_cross_entropy's
 * loop, charmodel-predict.c:62-76; with skip >= len - 1 it is rnn_char_prime's loop,
 * 407-416); otherwise the row is output_size / alphabet_len heads and sums[c] gets head
 * c's sum (rnn_char_multi_cross_entropy's loop, charmodel-multi-predict.c:388-403).
 * The net's state rows stay on the device. */
static void run_text(RecurNN *net, const u8 *text, int len, int skip, int alphabet_len,
                     double *sums, int n_sums) {
  RamdEngine *e = ramd_engine_of(net);
  RamdPriv *p = ramd_priv(net);
  ramd_engine_ensure_device(e);
  ramd_engine_need_dev(e, RNN_AMD_WEIGHTS);
  ramd_stream_need_dev(e, net);
  for (int c = 0; c < n_sums; c++) {
    sums[c] = 0.0;
  }
  if (len < 2) {
    return;
  }
  const RamdShape *s = &e->sh;
  int r = ramd_state_row(e, p);
  unsigned char *d_text = ramd_dev_alloc(len);
  double *d_acc = alphabet_len ? ramd_dev_alloc((size_t)n_sums * sizeof(double)) : NULL;
  ramd_h2d(d_text, text, len);
  HIP_OK(hipMemsetAsync(e->b.xent + r, 0, sizeof(double), ramd_stream));
  if (p->stream >= 0) {
    ramd_h2d(e->b.idx + p->stream, &net->bptt->index, sizeof(int));
  }
  ramd_dsync();
  unsigned char *old_text = e->b.text;
  int old_len = e->b.text_len;
  e->b.text = d_text;
  e->b.text_len = len;
  ramd_set_uniform_idx(e, p->stream >= 0 ? p->stream : e->n_streams, p->stream >= 0 ? 1 : 0);
  for (int i = 0; i < len - 1; i++) {
    const RamdFwdCall call = {.row0 = r, .nrows = 1, .mode = RAMD_IN_TEXT, .text_i = i, .global_count = 1};
    ramd_launch_forward(ramd_stream, s, &e->b, &call, NULL, NULL);
    if (alphabet_len) {
      if (i >= skip) {
        ramd_launch_multi_xent_accumulate(ramd_stream, s, &e->b, r, alphabet_len, n_sums, d_acc, 1);
      }
    } else {
      ramd_launch_xent_accumulate(ramd_stream, s, &e->b, r, i >= skip);
    }
  }
  if (alphabet_len) {
    ramd_d2h(sums, d_acc, (size_t)n_sums * sizeof(double));
  } else {
    ramd_d2h(sums, e->b.xent + r, sizeof(double));
  }
  ramd_dsync();
  e->b.text = old_text;
  e->b.text_len = old_len;
  ramd_dev_free(d_text);
  ramd_dev_free(d_acc);
  p->dev_valid = 1;
  p->host_valid = 0;
}

double rnn_amd_run_text(RecurNN *net, const u8 *text, int len, int skip) {
  double sum = 0.0;
  run_text(net, text, len, skip, 0, &sum, 1);
  return sum;
}

void rnn_amd_run_text_heads(RecurNN *net, const u8 *text, int len, int skip, int alphabet_len,
                            double *sums) {
  int n_classes = alphabet_len > 0 ? net->output_size / alphabet_len : 0;
  if (n_classes < 1) {
    fprintf(stderr, "librecur_amd: rnn_amd_run_text_heads: %d outputs as heads of %d\n",
            net->output_size, alphabet_len);
    abort();
  }
  run_text(net, text, len, skip, alphabet_len, sums, n_classes);
}
