/* engine.c -- the device and engine layer of the RNN core's host side (gnu11 C): the device and the library's stream,
 * the mailbox of small uploads and downloads, the life cycle of a RamdEngine and the coherence protocol.  The structs
 * the caller sees are host memory, as the ABI demands; the device holds the authoritative copy of anything that has
 * been computed on.  There is no CPU implementation of the arithmetic: without a HIP device every compute entry point
 * aborts (ramd_require_device). */
#define RAMD_HIP_HOST 1
#include "rnn_host.h"
#include "coop_rule.h"

static int g_device = -1;      /* -1: not initialised */
static int g_device_count = -1;
hipStream_t ramd_stream = NULL;
static RamdEngine *g_engines = NULL;

/* ------------------------------------------------------------------ device -- */

int rnn_amd_device_count(void) {
  if (g_device_count < 0) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
      n = 0;
    }
    g_device_count = n;
  }
  return g_device_count;
}

void ramd_require_device(const char *what) {
  if (rnn_amd_device_count() <= 0) {
    fprintf(stderr,
            "librecur_amd: %s needs a HIP device (gfx950) and none is visible; "
            "this library has no CPU fallback\n",
            what);
    abort();
  }
  if (g_device < 0) {
    int dev = 0;
    const char *lr = getenv("LOCAL_RANK");
    if (lr && *lr) {
      dev = atoi(lr) % rnn_amd_device_count();
    }
    HIP_OK(hipSetDevice(dev));
    g_device = dev;
  }
}

void rnn_amd_use_device(int device, void *hip_stream) {
  if (rnn_amd_device_count() <= 0) {
    ramd_require_device("rnn_amd_use_device");
  }
  HIP_OK(hipSetDevice(device));
  g_device = device;
  ramd_stream = (hipStream_t)hip_stream;
}

void *rnn_amd_current_stream(void) { return (void *)ramd_stream; }
const char *rnn_amd_version(void) { return "recur_amd 0.1 (gfx950, fp32 MFMA)"; }
void rnn_amd_synchronize(void) {
  if (g_device >= 0) {
    ramd_dsync();
    HIP_OK(hipDeviceSynchronize());
  }
}
void rnn_amd_kernel_time_enable(int enable) { ramd_timing_enable(enable); }
long rnn_amd_fwd_top_launches(void) { return ramd_fwd_top_launches(); }
long rnn_amd_chain_early_launches(void) { return ramd_chain_early_launches(); }
double rnn_amd_kernel_time_ms(int which, long *launches, int reset) {
  return ramd_timing_ms(which, launches, reset);
}

void *ramd_dev_alloc(size_t bytes) {
  void *p = NULL;
  if (bytes == 0) {
    bytes = 16;
  }
  HIP_OK(hipMalloc(&p, bytes));
  HIP_OK(hipMemsetAsync(p, 0, bytes, ramd_stream));
  return p;
}
/* The arrays that PEERS read and write in the kernel-issued exchange (weights, delta sums): RECUR_AMD_XCHG_FINEGRAINED=1
 * makes them fine-grained device allocations (hipExtMallocWithFlags: coherent between devices inside a kernel, not only
 * at kernel boundaries) -- for a node on which bench.py's start-up cross-check finds the coarse-grained default's
 * replicas differing (nothing of the kind has been seen: no multi-GPU node has run this yet).
 * Costs the owner's own kernels their L2 for these arrays (measured on one GPU: profiles/NOTES_r06.md). */
static void *dev_alloc_exchanged(size_t bytes) {
  static int fine = -1;
  if (fine < 0) {
    const char *v = getenv("RECUR_AMD_XCHG_FINEGRAINED");
    fine = v && *v == '1';
  }
  if (!fine) {
    return ramd_dev_alloc(bytes);
  }
  void *p = NULL;
  HIP_OK(hipExtMallocWithFlags(&p, bytes ? bytes : 16, hipDeviceMallocFinegrained));
  HIP_OK(hipMemsetAsync(p, 0, bytes ? bytes : 16, ramd_stream));
  return p;
}
void ramd_dev_free(void *p) {
  if (p) {
    HIP_OK(hipFree(p));
  }
}
void ramd_h2d(void *d, const void *h, size_t bytes) {
  if (bytes) {
    HIP_OK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, ramd_stream));
  }
}
void ramd_d2h(void *h, const void *d, size_t bytes) {
  if (bytes) {
    HIP_OK(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, ramd_stream));
  }
}
static unsigned long g_syncs = 0; /* completed stream synchronisations */
void ramd_dsync(void) {
  HIP_OK(hipStreamSynchronize(ramd_stream));
  g_syncs++;
  if (ramd_chain_abort_word()) {
    const unsigned code = ramd_chain_abort_word();
    if (code == COOP_ABORT_XCHG_BARRIER) {
      fprintf(stderr, "librecur_amd: a rank waited its time out (20 s; RECUR_AMD_XCHG_BARRIER_TIMEOUT_S) at a barrier of the kernel-issued exchange: not every rank "
                      "reached it (did one die, or drive fewer generations?); the replicas are out of step.\n");
    } else if (code == COOP_ABORT_FWD_TOP) {
      fprintf(stderr, "librecur_amd: the text step's forward + top launch gave up (code 7: its 256 workgroups were not all "
                      "resident, one per CU, or a hand-off timed out); its results are invalid.  Set RECUR_AMD_FWD_TOP=0 "
                      "(the two launches).\n");
    } else if (code == COOP_ABORT_CHAIN_OFF_XCD) {
      fprintf(stderr, "librecur_amd: a workgroup of the one-launch BPTT chain was not on the XCD its number implies (code 2): "
                      "something else ran on this GPU beside the chain and the dispatcher interleaved the two launches; "
                      "its results are invalid.  That form is only taken with RECUR_AMD_XCD_STATIC=1: drop it (the default "
                      "takes the seat from the CU a workgroup runs on, whatever runs beside it).\n");
    } else { /* COOP_ABORT_CHAIN */
      fprintf(stderr, "librecur_amd: the one-launch BPTT chain gave up (code %u: its 256 workgroups were "
                      "not all resident, one per CU, or a hand-off timed out); its results are invalid.  "
                      "Set RECUR_AMD_CHAIN_CHECK=1 (every launch checked, a chain that gives up is redone) or "
                      "RECUR_AMD_CHAIN_PERSIST=0 (the launch-per-step chain).\n", code);
    }
    abort();
  }
}

/* ---------------------------------------------------------------- mailbox -- */

/* The per-net calls move a handful of small vectors each way (the caller's inputs or output
 * error in; the layers, the error images and two scalars out).  As separate hipMemcpyAsync
 * calls on pageable memory each of them costs a staging copy and an implicit wait; here they
 * are queued, carried by ONE kernel launch per direction through a pinned, device-mapped
 * mailbox, and a call ends with one stream synchronisation.  ramd_mail_in snapshots the host
 * data at once (the caller may change it as soon as we return), ramd_mail_out delivers after
 * the synchronisation in ramd_mail_out_flush. */
#define MAIL_SEGS 12
#define MAIL_WORDS (1u << 18) /* per direction: 1 MB */
static struct {
  unsigned *buf; /* [2][MAIL_WORDS] pinned: inbound half, outbound half */
  void *dst[MAIL_SEGS];
  const void *src[MAIL_SEGS];
  unsigned n[MAIL_SEGS];
  int nseg;
  unsigned cur;
  unsigned long in_sync; /* g_syncs when the inbound half was last handed to the device */
  int in_busy;
} g_mail;

static void mail_ready(void) {
  if (!g_mail.buf) {
    HIP_OK(hipHostMalloc((void **)&g_mail.buf, 2 * (size_t)MAIL_WORDS * sizeof(unsigned),
                         hipHostMallocPortable | hipHostMallocMapped));
  }
}
void ramd_mail_in_flush(void) {
  if (g_mail.nseg) {
    ramd_launch_segcopy(ramd_stream, g_mail.nseg, g_mail.dst, g_mail.src, g_mail.n);
    g_mail.nseg = 0;
    g_mail.in_busy = 1;
    g_mail.in_sync = g_syncs;
  }
}
void ramd_mail_in(void *dev, const void *host, size_t bytes) {
  unsigned words = (unsigned)(bytes / 4);
  if (!bytes) {
    return;
  }
  mail_ready();
  if ((bytes & 3) || words > MAIL_WORDS) { /* not this route's kind of copy */
    ramd_mail_in_flush();
    ramd_h2d(dev, host, bytes);
    ramd_dsync(); /* the caller's buffer is its own again when we return */
    return;
  }
  if (g_mail.nseg == 0 && g_mail.in_busy) {
    /* the inbound half may still be being read by the launch that carried the last batch */
    if (g_mail.in_sync == g_syncs && g_mail.cur + words > MAIL_WORDS) {
      ramd_dsync();
    }
    if (g_mail.in_sync != g_syncs) {
      g_mail.in_busy = 0;
      g_mail.cur = 0;
    }
  }
  if (g_mail.nseg == MAIL_SEGS || g_mail.cur + words > MAIL_WORDS) {
    ramd_mail_in_flush();
    ramd_dsync();
    g_mail.in_busy = 0;
    g_mail.cur = 0;
  }
  unsigned *slot = g_mail.buf + g_mail.cur;
  memcpy(slot, host, bytes);
  g_mail.dst[g_mail.nseg] = dev;
  g_mail.src[g_mail.nseg] = slot;
  g_mail.n[g_mail.nseg] = words;
  g_mail.nseg++;
  g_mail.cur += words;
}
/* outbound: queue, then one launch + one synchronisation + the deliveries */
static struct {
  void *dst[MAIL_SEGS];
  const void *src[MAIL_SEGS];
  unsigned n[MAIL_SEGS];
  void *host[MAIL_SEGS];
  int nseg;
  unsigned cur;
} g_mail_out;
void ramd_mail_out_flush(void) {
  ramd_mail_in_flush();
  if (g_mail_out.nseg) {
    ramd_launch_segcopy(ramd_stream, g_mail_out.nseg, g_mail_out.dst, g_mail_out.src, g_mail_out.n);
  }
  ramd_dsync();
  for (int g = 0; g < g_mail_out.nseg; g++) {
    memcpy(g_mail_out.host[g], g_mail_out.dst[g], (size_t)g_mail_out.n[g] * 4);
  }
  g_mail_out.nseg = 0;
  g_mail_out.cur = 0;
}
void ramd_mail_out(void *host, const void *dev, size_t bytes) {
  unsigned words = (unsigned)(bytes / 4);
  if (!bytes) {
    return;
  }
  mail_ready();
  if ((bytes & 3) || words > MAIL_WORDS) {
    ramd_d2h(host, dev, bytes); /* completes with the synchronisation of the flush */
    return;
  }
  if (g_mail_out.nseg == MAIL_SEGS || g_mail_out.cur + words > MAIL_WORDS) {
    ramd_mail_out_flush();
  }
  unsigned *slot = g_mail.buf + MAIL_WORDS + g_mail_out.cur;
  g_mail_out.dst[g_mail_out.nseg] = slot;
  g_mail_out.src[g_mail_out.nseg] = dev;
  g_mail_out.n[g_mail_out.nseg] = words;
  g_mail_out.host[g_mail_out.nseg] = host;
  g_mail_out.nseg++;
  g_mail_out.cur += words;
}

/* The set calls' small per-generation uploads (symbols, targets, dense input rows): snapshot into
 * the pinned mailbox and carried by a launch on the stream -- the caller's buffer is free when we
 * return and nobody waits for the device; what does not fit or is not word-sized goes the old way
 * (copy, then wait).  rows of `width` bytes, `host_pitch` apart, land contiguously at `dev`. */
void ramd_upload_rows_q(void *dev, const void *host, size_t host_pitch, size_t width, size_t rows, int flush) {
  size_t bytes = width * rows;
  if (!bytes) {
    return;
  }
  mail_ready();
  if ((bytes & 3) || bytes / 4 > MAIL_WORDS) {
    ramd_mail_in_flush();
    if (host_pitch == width) {
      ramd_h2d(dev, host, bytes);
    } else {
      HIP_OK(hipMemcpy2DAsync(dev, width, host, host_pitch, width, rows, hipMemcpyHostToDevice, ramd_stream));
    }
    ramd_dsync();
    return;
  }
  if (host_pitch == width) {
    ramd_mail_in(dev, host, bytes);
  } else {
    /* pack the rows behind one another in the mailbox: one segment */
    unsigned words = (unsigned)(bytes / 4);
    if (g_mail.nseg == 0 && g_mail.in_busy && g_mail.in_sync != g_syncs) {
      g_mail.in_busy = 0;
      g_mail.cur = 0;
    }
    if (g_mail.nseg == MAIL_SEGS || g_mail.cur + words > MAIL_WORDS) {
      ramd_mail_in_flush();
      ramd_dsync();
      g_mail.in_busy = 0;
      g_mail.cur = 0;
    }
    unsigned *slot = g_mail.buf + g_mail.cur;
    for (size_t r = 0; r < rows; r++) {
      memcpy((char *)slot + r * width, (const char *)host + r * host_pitch, width);
    }
    g_mail.dst[g_mail.nseg] = dev;
    g_mail.src[g_mail.nseg] = slot;
    g_mail.n[g_mail.nseg] = words;
    g_mail.nseg++;
    g_mail.cur += words;
  }
  if (flush) {
    ramd_mail_in_flush();
  }
}
void ramd_upload_rows(void *dev, const void *host, size_t host_pitch, size_t width, size_t rows) {
  ramd_upload_rows_q(dev, host, host_pitch, width, rows, 1);
}
void ramd_upload(void *dev, const void *host, size_t bytes) { ramd_upload_rows_q(dev, host, bytes, bytes, 1, 1); }
/* queued: leaves with the next ramd_upload() / ramd_mail_in_flush() */
void ramd_upload_q(void *dev, const void *host, size_t bytes) { ramd_upload_rows_q(dev, host, bytes, bytes, 1, 0); }

void *ramd_zalloc(size_t bytes) {
  void *p = NULL;
  if (posix_memalign(&p, 64, bytes ? bytes : 64)) {
    fprintf(stderr, "librecur_amd: cannot allocate %zu bytes\n", bytes);
    abort(); /* recur-common.h:95-132: allocation failure aborts */
  }
  memset(p, 0, bytes ? bytes : 64);
  return p;
}

/* ----------------------------------------------------------------- engines -- */

RamdEngine *ramd_engine_new(RecurNN *owner) {
  RamdEngine *e = ramd_zalloc(sizeof(RamdEngine));
  e->owner = owner;
  e->sh.input_size = owner->input_size;
  e->sh.hidden_size = owner->hidden_size;
  e->sh.output_size = owner->output_size;
  e->sh.I = owner->i_size;
  e->sh.H = owner->h_size;
  e->sh.O = owner->o_size;
  e->sh.activation = owner->activation;
  e->ih_size = (size_t)owner->ih_size;
  e->ho_size = (size_t)owner->ho_size;
  e->host_valid = RNN_AMD_WEIGHTS | RNN_AMD_MOMENTUMS | RNN_AMD_DELTAS;
  noise_ahead_reset(&e->ahead);
  e->next = g_engines;
  g_engines = e;
  return e;
}

static void engine_free_device(RamdEngine *e) {
  if (!e->dev_ready) {
    return;
  }
  RamdBuffers *b = &e->b;
  ramd_noise_ahead_free_device(e);
  ramd_dev_free(b->ih_w); ramd_dev_free(b->ho_w); ramd_dev_free(b->ih_m); ramd_dev_free(b->ho_m);
  ramd_dev_free(b->ih_aux); ramd_dev_free(b->ho_aux); ramd_dev_free(e->delta_own);
  ramd_dev_free(b->arena); ramd_dev_free(b->hidden); ramd_dev_free(b->out); ramd_dev_free(b->o_error);
  ramd_dev_free(b->err_a); ramd_dev_free(b->err_b); ramd_dev_free(b->ehi); ramd_dev_free(b->esum);
  ramd_dev_free(b->coef); ramd_dev_free(b->ex); ramd_dev_free(b->esum_part); ramd_dev_free(b->zeros); ramd_dev_free(b->ones); ramd_dev_free(b->rng); ramd_dev_free(b->slab); ramd_dev_free(b->ho_slab); ramd_dev_free(b->idx); ramd_dev_free(b->lr); ramd_dev_free(b->mef);
  ramd_dev_free(b->ih_scale); ramd_dev_free(b->top_raw); ramd_dev_free(b->top_scaled); ramd_dev_free(b->bptt_err);
  ramd_dev_free(b->n_exec); ramd_dev_free(b->depth_log); ramd_dev_free(b->target); ramd_dev_free(b->hot);
  ramd_dev_free(b->xent);
  ramd_dev_free(b->active); ramd_dev_free(b->stat_err); ramd_dev_free(b->stat_ent); ramd_dev_free(b->stat_zero);
  ramd_dev_free(b->stat_depth); ramd_dev_free(b->stat_correct); ramd_dev_free(b->stat_count);
  ramd_dev_free(b->text);
  ramd_dev_free(b->bw); ramd_dev_free(b->bm); ramd_dev_free(b->baux); ramd_dev_free(b->bdelta);
  ramd_dev_free(b->binp); ramd_dev_free(b->bout); ramd_dev_free(b->berr); ramd_dev_free(b->bcarry); ramd_dev_free(b->blast);
  ramd_dev_free(e->d_scratch); ramd_dev_free(e->d_ranges); ramd_dev_free(e->d_dense);
  ramd_dev_free(e->d_mranges); ramd_dev_free(e->d_mclass); ramd_dev_free(e->d_group);
  ramd_dev_free(b->mheads_part);
  b->mheads_part = NULL;
  b->mheads_part_floats = 0;
  free(e->active_host); /* (b.active goes with the device arrays) */
  e->active_host = NULL;
  e->active_host_n = 0;
  free(e->top_done_mask); /* (sized by Scap, which may grow) */
  e->top_done_mask = NULL;
  e->top_done = 0;
  ramd_dev_free(e->d_kept_slab);
  e->d_kept_slab = NULL;
  e->kept_floats = 0;
  e->kept_live = 0;
  e->d_group = NULL;
  e->d_group_bytes = 0;
  ramd_dev_free(e->d_block);
  e->d_block = NULL;
  e->d_block_bytes = 0;
  e->d_mranges = NULL;
  e->d_mclass = NULL;
  free(e->lr_pushed);
  e->lr_pushed = NULL;
  free(e->idx_pushed);
  e->idx_pushed = NULL;
  memset(b, 0, sizeof(*b));
  e->delta_own = NULL;
  e->delta_external = 0;
  e->dev_ready = 0;
}

void ramd_engine_delete(RamdEngine *e) {
  if (g_device >= 0) {
    ramd_dsync();
  }
  engine_free_device(e);
  ramd_noise_ahead_destroy(e);
  /* clones may outlive the net that owns the weights (text-predict.c:654-656 deletes the
   * training set, then its confab and validation clones): detach them so that their own
   * rnn_delete_net finds no engine instead of a freed one */
  for (int i = 0; i < e->n_streams; i++) {
    if (e->streams[i] && e->streams[i] != e->owner) {
      RamdPriv *q = ramd_priv(e->streams[i]);
      q->eng = NULL;
      q->stream = q->fwd = -1;
    }
  }
  for (int i = 0; i < e->n_fwd; i++) {
    if (e->fwd[i] && e->fwd[i] != e->owner) {
      RamdPriv *q = ramd_priv(e->fwd[i]);
      q->eng = NULL;
      q->stream = q->fwd = -1;
    }
  }
  RamdEngine **pp = &g_engines;
  while (*pp && *pp != e) {
    pp = &(*pp)->next;
  }
  if (*pp) {
    *pp = e->next;
  }
  free(e->streams);
  free(e->fwd);
  free(e);
}

void ramd_engine_attach(RamdEngine *e, RecurNN *net) {
  RamdPriv *p = ramd_priv(net);
  p->eng = e;
  p->host_valid = 1;
  p->dev_valid = 0;
  if (net->bptt) {
    if (e->n_streams == 0) {
      e->sh.D = net->bptt->depth;
    } else if (net->bptt->depth != e->sh.D) {
      fprintf(stderr, "librecur_amd: nets sharing weights must share the BPTT depth (%d vs %d)\n",
              net->bptt->depth, e->sh.D);
      abort();
    }
    if (e->n_streams == e->cap_streams) {
      e->cap_streams = e->cap_streams ? e->cap_streams * 2 : 4;
      e->streams = realloc(e->streams, e->cap_streams * sizeof(RecurNN *));
    }
    p->stream = e->n_streams;
    p->fwd = -1;
    e->streams[e->n_streams++] = net;
  } else {
    if (e->n_fwd == e->cap_fwd) {
      e->cap_fwd = e->cap_fwd ? e->cap_fwd * 2 : 4;
      e->fwd = realloc(e->fwd, e->cap_fwd * sizeof(RecurNN *));
    }
    p->fwd = e->n_fwd;
    p->stream = -1;
    e->fwd[e->n_fwd++] = net;
  }
}

RamdEngine *ramd_engine_of(RecurNN *net) {
  RamdPriv *p = ramd_priv(net);
  if (!p->eng) {
    /* a net made by rnn_new without OWN_WEIGHTS whose caller pointed it at
     * somebody's weights by hand: find that somebody */
    for (RamdEngine *e = g_engines; e; e = e->next) {
      if (e->owner->ih_weights == net->ih_weights) {
        ramd_engine_attach(e, net);
        break;
      }
    }
    if (!p->eng) {
      fprintf(stderr, "librecur_amd: net %p has no weights known to the library\n", (void *)net);
      abort();
    }
  }
  return p->eng;
}

int ramd_state_row(const RamdEngine *e, const RamdPriv *p) {
  return p->stream >= 0 ? p->stream : e->sh.Scap + p->fwd;
}

/* -------------------------------------------- host <-> device: one stream -- */

/* A generator of this engine has been written from the host (a caller's draw, a per-net call's upload): nothing that was
 * generated ahead from the device's states can be right any more.  (The counts the two-ahead slots are stamped with are
 * PREDICTED -- one pass and one loss on -- so a different sequence of the same length, an upload instead of the loss,
 * would have been accepted had this only counted: ADVICE.md round 4.) */
void ramd_rng_written_from_host(RamdEngine *e) { noise_ahead_host_write(&e->ahead); }

void ramd_stream_copy(RamdEngine *e, RecurNN *net, int to_device) {
  RamdPriv *p = ramd_priv(net);
  const RamdShape *s = &e->sh;
  RamdBuffers *b = &e->b;
  int r = ramd_state_row(e, p);
  size_t I = s->I, H = s->H, O = s->O;
#define COPY(dptr, hptr, n)                                                        \
  do {                                                                             \
    if (to_device) ramd_h2d((dptr), (hptr), (n) * sizeof(float));                       \
    else ramd_d2h((hptr), (dptr), (n) * sizeof(float));                                 \
  } while (0)
  COPY(b->hidden + (size_t)r * H, net->hidden_layer, H);
  COPY(b->out + (size_t)r * O, net->output_layer, O);
  if (to_device) {
    ramd_h2d((char *)b->rng + (size_t)r * sizeof(rand_ctx), &net->rng, sizeof(rand_ctx));
    ramd_rng_written_from_host(e);
  } else {
    ramd_d2h(&net->rng, (char *)b->rng + (size_t)r * sizeof(rand_ctx), sizeof(rand_ctx));
  }
  if (p->stream >= 0) {
    RecurNNBPTT *bp = net->bptt;
    int j = p->stream;
    /* history: host [D][I] per net <-> device [D][Scap][I] */
    if (to_device) {
      HIP_OK(hipMemcpy2DAsync(b->arena + (size_t)j * I, (size_t)s->Scap * I * sizeof(float),
                              bp->history, I * sizeof(float), I * sizeof(float), s->D,
                              hipMemcpyHostToDevice, ramd_stream));
    } else {
      HIP_OK(hipMemcpy2DAsync(bp->history, I * sizeof(float), b->arena + (size_t)j * I,
                              (size_t)s->Scap * I * sizeof(float), I * sizeof(float), s->D,
                              hipMemcpyDeviceToHost, ramd_stream));
    }
    COPY(b->o_error + (size_t)j * O, bp->o_error, O);
    COPY(b->err_a + (size_t)j * I, bp->h_error, I);
    COPY(b->err_b + (size_t)j * I, bp->i_error, I);
    COPY(b->mef + j, &bp->min_error_factor, 1);
    COPY(b->ih_scale + j, &bp->ih_scale, 1);
    if (to_device) {
      ramd_h2d(b->idx + j, &bp->index, sizeof(int));
      ramd_h2d(b->lr + j, &bp->learn_rate, sizeof(float));
      e->lr_pushed[j] = bp->learn_rate;
      e->idx_pushed[j] = bp->index;
    }
  } else {
    COPY(b->arena + ((size_t)s->D * s->Scap + p->fwd) * I, net->input_layer, I);
  }
#undef COPY
}

void ramd_err_flush(RamdEngine *e) {
  if (e->err_pending) {
    ramd_launch_err_writeback(ramd_stream, &e->sh, &e->b, e->err_row0, e->err_nrows);
    e->err_pending = 0;
  }
}

/* after a ramd_launch_calc_deltas over these rows: their error images wait for k_err_writeback, unless the launch left
 * them itself (the one-workgroup BPTT of a small net) */
void ramd_err_after_calc(RamdEngine *e, int row0, int nrows) {
  e->err_pending = !ramd_calc_wrote_images();
  e->err_row0 = row0;
  e->err_nrows = nrows;
}

void ramd_stream_need_host(RamdEngine *e, RecurNN *net) {
  RamdPriv *p = ramd_priv(net);
  if (!p->host_valid && e->dev_ready) {
    ramd_err_flush(e);
    ramd_stream_copy(e, net, 0);
    ramd_dsync();
  }
  p->host_valid = 1;
}

void ramd_stream_need_dev(RamdEngine *e, RecurNN *net) {
  RamdPriv *p = ramd_priv(net);
  if (!p->dev_valid) {
    ramd_stream_copy(e, net, 1);
    ramd_dsync(); /* the host arrays may change as soon as we return */
    ramd_top_done_clear(e);
  }
  p->dev_valid = 1;
}

/* ------------------------------------------- host <-> device: the big arrays -- */

/* rnn_bptt_clear_deltas is lazy: the callers that clear per generation (gstclassify, rnnca) go on
 * with an accumulating rnn_bptt_calc_deltas, which can just as well not accumulate -- two memset
 * launches less.  Whoever else needs the delta arrays gets the zeros first. */
void ramd_deltas_materialize(RamdEngine *e) {
  if (e->kept_live) { /* (never together with a pending clear: whichever came later dropped the other) */
    e->kept_live = 0;
    if (e->dev_ready) {
      ramd_launch_pending_finalize(ramd_stream, &e->kept);
    }
  }
  if (e->deltas_zero_pending) {
    e->deltas_zero_pending = 0;
    if (e->dev_ready) {
      ramd_launch_clear_deltas(ramd_stream, &e->sh, &e->b);
    }
  }
}

void ramd_engine_need_host(RamdEngine *e, int what) {
  if (what & RNN_AMD_DELTAS) {
    ramd_deltas_materialize(e);
  }
  RecurNN *o = e->owner;
  RecurExtraLayer *bl = e->sh.bI ? o->bottom_layer : NULL;
  size_t bn = (size_t)e->sh.bI * e->sh.bO;
  int fetch = what & ~e->host_valid & (RNN_AMD_WEIGHTS | RNN_AMD_MOMENTUMS | RNN_AMD_DELTAS);
  if (fetch && e->dev_ready) {
    if (fetch & RNN_AMD_WEIGHTS) {
      ramd_d2h(o->ih_weights, e->b.ih_w, e->ih_size * sizeof(float));
      ramd_d2h(o->ho_weights, e->b.ho_w, e->ho_size * sizeof(float));
      if (bl) ramd_d2h(bl->weights, e->b.bw, bn * sizeof(float));
    }
    if ((fetch & RNN_AMD_MOMENTUMS) && bl) {
      ramd_d2h(bl->momentums, e->b.bm, bn * sizeof(float));
      if (bl->aux) ramd_d2h(bl->aux, e->b.baux, bn * sizeof(float));
    }
    if ((fetch & RNN_AMD_DELTAS) && bl) {
      ramd_d2h(bl->delta, e->b.bdelta, bn * sizeof(float));
      ramd_d2h(bl->o_error, e->b.bcarry + (size_t)e->b.bcarry_cur * e->sh.bO, e->sh.bO * sizeof(float));
    }
    if ((fetch & RNN_AMD_MOMENTUMS) && o->bptt) {
      if (e->has_momentum) {
        ramd_d2h(o->bptt->ih_momentum, e->b.ih_m, e->ih_size * sizeof(float));
        ramd_d2h(o->bptt->ho_momentum, e->b.ho_m, e->ho_size * sizeof(float));
      }
      if (e->has_aux) {
        ramd_d2h(o->bptt->ih_aux, e->b.ih_aux, e->ih_size * sizeof(float));
        ramd_d2h(o->bptt->ho_aux, e->b.ho_aux, e->ho_size * sizeof(float));
      }
    }
    if ((fetch & RNN_AMD_DELTAS) && o->bptt && e->has_delta) {
      ramd_d2h(o->bptt->ih_delta, e->b.ih_delta, e->ih_size * sizeof(float));
      ramd_d2h(o->bptt->ho_delta, e->b.ho_delta, e->ho_size * sizeof(float));
    }
    ramd_dsync();
  }
  e->host_valid |= fetch;
}

void ramd_engine_need_dev(RamdEngine *e, int what) {
  if (what & RNN_AMD_DELTAS) {
    ramd_deltas_materialize(e);
  }
  RecurNN *o = e->owner;
  RecurExtraLayer *bl = e->sh.bI ? o->bottom_layer : NULL;
  size_t bn = (size_t)e->sh.bI * e->sh.bO;
  int push = what & ~e->dev_valid & (RNN_AMD_WEIGHTS | RNN_AMD_MOMENTUMS | RNN_AMD_DELTAS);
  if (!push) {
    return;
  }
  ramd_top_done_clear(e);
  if (push & RNN_AMD_WEIGHTS) {
    ramd_h2d(e->b.ih_w, o->ih_weights, e->ih_size * sizeof(float));
    ramd_h2d(e->b.ho_w, o->ho_weights, e->ho_size * sizeof(float));
    if (bl) ramd_h2d(e->b.bw, bl->weights, bn * sizeof(float));
  }
  if ((push & RNN_AMD_MOMENTUMS) && bl) {
    ramd_h2d(e->b.bm, bl->momentums, bn * sizeof(float));
    if (bl->aux) ramd_h2d(e->b.baux, bl->aux, bn * sizeof(float));
  }
  if ((push & RNN_AMD_DELTAS) && bl) {
    ramd_h2d(e->b.bdelta, bl->delta, bn * sizeof(float));
    ramd_h2d(e->b.bcarry + (size_t)e->b.bcarry_cur * e->sh.bO, bl->o_error, e->sh.bO * sizeof(float));
  }
  if ((push & RNN_AMD_MOMENTUMS) && o->bptt) {
    if (e->has_momentum) {
      ramd_h2d(e->b.ih_m, o->bptt->ih_momentum, e->ih_size * sizeof(float));
      ramd_h2d(e->b.ho_m, o->bptt->ho_momentum, e->ho_size * sizeof(float));
    }
    if (e->has_aux) {
      ramd_h2d(e->b.ih_aux, o->bptt->ih_aux, e->ih_size * sizeof(float));
      ramd_h2d(e->b.ho_aux, o->bptt->ho_aux, e->ho_size * sizeof(float));
    }
  }
  if ((push & RNN_AMD_DELTAS) && o->bptt && e->has_delta) {
    ramd_h2d(e->b.ih_delta, o->bptt->ih_delta, e->ih_size * sizeof(float));
    ramd_h2d(e->b.ho_delta, o->bptt->ho_delta, e->ho_size * sizeof(float));
  }
  ramd_dsync();
  e->dev_valid |= push;
}

void ramd_engine_dev_wrote(RamdEngine *e, int what) {
  e->dev_valid |= what;
  e->host_valid &= ~what;
  if (what & RNN_AMD_WEIGHTS) {
    ramd_top_done_clear(e);
  }
}

/* public: bring host copies up to date */
void ramd_need_host(RecurNN *net, int what) {
  RamdEngine *e = ramd_engine_of(net);
  ramd_engine_need_host(e, what);
  if (what & RNN_AMD_ALL_STREAMS) {
    for (int i = 0; i < e->n_streams; i++) {
      ramd_stream_need_host(e, e->streams[i]);
    }
    for (int i = 0; i < e->n_fwd; i++) {
      ramd_stream_need_host(e, e->fwd[i]);
    }
  } else if (what & RNN_AMD_STREAM) {
    ramd_stream_need_host(e, net);
  }
}

void ramd_host_wrote(RecurNN *net, int what) {
  RamdEngine *e = ramd_engine_of(net);
  int big = what & (RNN_AMD_WEIGHTS | RNN_AMD_MOMENTUMS | RNN_AMD_DELTAS);
  /* a partial host write on top of a stale host copy would lose the rest */
  ramd_engine_need_host(e, big);
  e->host_valid |= big;
  e->dev_valid &= ~big;
  if (what & RNN_AMD_ALL_STREAMS) {
    for (int i = 0; i < e->n_streams; i++) {
      ramd_stream_need_host(e, e->streams[i]);
      ramd_priv(e->streams[i])->dev_valid = 0;
    }
    for (int i = 0; i < e->n_fwd; i++) {
      ramd_stream_need_host(e, e->fwd[i]);
      ramd_priv(e->fwd[i])->dev_valid = 0;
    }
  } else if (what & RNN_AMD_STREAM) {
    ramd_stream_need_host(e, net);
    ramd_priv(net)->dev_valid = 0;
  }
}

/* A host-side draw from net->rng (charmodel-predict.c:52, 93) while the stream's state
 * lives on the device: fetch only the generator before, push only it back after. */
void ramd_rng_to_host(RecurNN *net) {
  RamdPriv *p = ramd_priv(net);
  RamdEngine *e = p->eng;
  if (e && e->dev_ready && p->dev_valid && !p->host_valid) {
    ramd_d2h(&net->rng, (char *)e->b.rng + (size_t)ramd_state_row(e, p) * sizeof(rand_ctx), sizeof(rand_ctx));
    ramd_dsync();
  }
}
void ramd_rng_from_host(RecurNN *net) {
  RamdPriv *p = ramd_priv(net);
  RamdEngine *e = p->eng;
  if (e && e->dev_ready && p->dev_valid) {
    ramd_h2d((char *)e->b.rng + (size_t)ramd_state_row(e, p) * sizeof(rand_ctx), &net->rng, sizeof(rand_ctx));
    ramd_rng_written_from_host(e);
    ramd_dsync();
  }
}

void rnn_amd_sync_host(RecurNN *net, int what) { ramd_need_host(net, what); }
void rnn_amd_host_written(RecurNN *net, int what) { ramd_host_wrote(net, what); }

/* Allocate (or grow) the device image.  Growing evicts everything to the host
 * first and starts over; it only happens when nets are cloned after the first
 * device call, or when rnn_amd_run_texts asks for more scratch rows than before. */
void ramd_engine_ensure_device(RamdEngine *e) {
  ramd_require_device("this call");
  /* the bottom layer is attached after rnn_new returns (recur-nn-init.c:215) */
  RecurExtraLayer *obl = e->owner->bottom_layer;
  int bI = obl ? obl->i_size : 0, bO = obl ? obl->o_size : 0;
  if (obl && (obl->output_size != e->sh.input_size || bI < 4 || bO < 4)) {
    fprintf(stderr, "librecur_amd: bottom layer of %d outputs under a net of %d inputs\n",
            obl->output_size, e->sh.input_size);
    abort();
  }
  int same_bottom = bI == e->sh.bI && bO == e->sh.bO;
  if (e->dev_ready && e->sh.Scap >= e->n_streams && e->sh.Fcap >= e->n_fwd + e->scratch_fwd && same_bottom) {
    return;
  }
  if (e->dev_ready && e->xchg_world) {
    fprintf(stderr, "librecur_amd: the device image has to grow (a clone made after rnn_amd_set_exchange_join?) while "
                    "other ranks hold pointers into it; leave the exchange first\n");
    abort();
  }
  unsigned char *keep_text = NULL;
  int keep_text_len = 0;
  float *keep_ext = NULL;
  if (e->dev_ready) {
    ramd_engine_need_host(e, RNN_AMD_WEIGHTS | RNN_AMD_MOMENTUMS | RNN_AMD_DELTAS);
    for (int i = 0; i < e->n_streams; i++) {
      RamdPriv *p = ramd_priv(e->streams[i]);
      if (p->dev_valid && !p->host_valid) {
        ramd_stream_need_host(e, e->streams[i]);
      }
    }
    for (int i = 0; i < e->n_fwd; i++) {
      RamdPriv *p = ramd_priv(e->fwd[i]);
      if (p->dev_valid && !p->host_valid) {
        ramd_stream_need_host(e, e->fwd[i]);
      }
    }
    ramd_dsync();
    /* what the caller registered with the engine survives the regrow: the text of the
     * host-free epoch loop and the external delta buffer of the multi-GPU path */
    if (e->b.text && e->b.text_len > 0) {
      keep_text_len = e->b.text_len;
      keep_text = malloc((size_t)keep_text_len);
      ramd_d2h(keep_text, e->b.text, (size_t)keep_text_len);
      ramd_dsync();
    }
    if (e->delta_external) {
      keep_ext = e->b.ih_delta;
    }
    engine_free_device(e);
  }
  RamdShape *s = &e->sh;
  RamdBuffers *b = &e->b;
  RecurNN *o = e->owner;
  s->bI = bI;
  s->bO = bO;
  s->b_in = obl ? obl->input_size : 0;
  s->b_out = obl ? obl->output_size : 0;
  s->Scap = (RAMD_MAX(e->n_streams, 1) + 15) / 16 * 16; /* whole 16-row tiles (k_chain_persist's PAD launches run over the rows above a set) */
  s->Fcap = RAMD_MAX(e->n_fwd + e->scratch_fwd, 1); /* the clones' rows, then the engine's scratch rows (rnn_amd_run_texts) */
  if (s->D < 1) {
    s->D = 1;
  }
  size_t I = s->I, H = s->H, O = s->O, S = s->Scap, F = s->Fcap, D = s->D;
  size_t fl = sizeof(float);
  if ((D + 1) * (S + F) * I >= ((size_t)1 << 31) || e->ih_size >= ((size_t)1 << 31)) {
    fprintf(stderr, "librecur_amd: %zu streams x depth %zu x %zu inputs exceeds the 2^31-element "
                    "offsets of the kernels\n", S, D, I);
    abort();
  }
  e->has_momentum = o->bptt && o->bptt->ih_momentum;
  e->has_aux = o->bptt && o->bptt->ih_aux;
  e->has_delta = o->bptt && o->bptt->ih_delta;
  b->ih_w = dev_alloc_exchanged(e->ih_size * fl);
  b->ho_w = dev_alloc_exchanged(e->ho_size * fl);
  b->ih_m = ramd_dev_alloc(e->ih_size * fl);
  b->ho_m = ramd_dev_alloc(e->ho_size * fl);
  if (e->has_aux) {
    b->ih_aux = ramd_dev_alloc(e->ih_size * fl);
    b->ho_aux = ramd_dev_alloc(e->ho_size * fl);
  }
  e->delta_own = dev_alloc_exchanged((e->ih_size + e->ho_size) * fl);
  b->ih_delta = e->delta_own;
  b->ho_delta = e->delta_own + e->ih_size;
  b->arena = ramd_dev_alloc(((D * S + F) * I + 128) * fl); /* + slack: k_delta_dma's rest tile reads up to 128 floats from column rows_core of the last row */
  b->hidden = ramd_dev_alloc((S + F) * H * fl);
  b->out = ramd_dev_alloc((S + F) * O * fl);
  b->o_error = ramd_dev_alloc(S * O * fl);
  b->err_a = ramd_dev_alloc(S * I * fl);
  b->err_b = ramd_dev_alloc(S * I * fl);
  b->ehi = ramd_dev_alloc((D + 1) * S * I * fl);
  b->esum = ramd_dev_alloc(D * S * fl);
  b->coef = ramd_dev_alloc(D * S * fl);
  {
    size_t nxp = ((size_t)(s->I - s->hidden_size) + 3) & ~(size_t)3;
    size_t tn = ((size_t)s->hidden_size + 31) / 32;
    b->ex = ramd_dev_alloc((D + 1) * S * nxp * fl);
    b->esum_part = ramd_dev_alloc(D * (tn + 1) * S * fl);
    b->zeros = ramd_dev_alloc(256);
    b->rng = ramd_dev_alloc((S + F) * sizeof(rand_ctx));
    b->ones = ramd_dev_alloc(S * fl);
    {
      float *one = malloc(S * fl);
      for (size_t i = 0; i < S; i++) one[i] = 1.0f;
      ramd_h2d(b->ones, one, S * fl);
      ramd_dsync();
      free(one);
    }
  }
  /* split-K workspace: up to 16 slabs of the largest GEMM output */
  {
    size_t per = RAMD_MAX(e->ih_size, RAMD_MAX((S + F) * I, (S + F) * H));
    per = RAMD_MAX(per, D * S * ((I - s->hidden_size + 3) & ~(size_t)3));
    b->slab_floats = per * 16;
    /* ... and at least ONE slab of the two outputs that scale with o_size (the top layer's delta
     * GEMM, the output layer of all rows): a narrow net with a very wide output layer (40 hidden
     * units under 56 heads of 35 symbols) has them larger than 16 of everything else */
    b->slab_floats = RAMD_MAX(b->slab_floats, RAMD_MAX(e->ho_size, (S + F) * O));
    b->slab = ramd_dev_alloc(b->slab_floats * fl);
    b->ho_slab = e->ho_size <= ((size_t)1 << 20) ? ramd_dev_alloc(8 * e->ho_size * fl) : NULL;
  }
  b->idx = ramd_dev_alloc(S * sizeof(int));
  b->lr = ramd_dev_alloc(S * fl);
  b->mef = ramd_dev_alloc(S * fl);
  b->ih_scale = ramd_dev_alloc(S * fl);
  b->top_raw = ramd_dev_alloc(S * fl);
  b->top_scaled = ramd_dev_alloc(S * fl);
  b->bptt_err = ramd_dev_alloc(S * fl);
  b->n_exec = ramd_dev_alloc(S * sizeof(int));
  b->depth_log = ramd_dev_alloc(S * sizeof(int));
  b->target = ramd_dev_alloc((S + F) * sizeof(int));
  b->xent = ramd_dev_alloc((S + F) * sizeof(double));
  b->hot = ramd_dev_alloc((S + F) * sizeof(int));
  b->active = ramd_dev_alloc(S);
  b->stat_err = ramd_dev_alloc(S * sizeof(double));
  b->stat_ent = ramd_dev_alloc(S * sizeof(double));
  b->stat_zero = ramd_dev_alloc(S * sizeof(double));
  b->stat_depth = ramd_dev_alloc(S * sizeof(double));
  b->stat_correct = ramd_dev_alloc(S * sizeof(long long));
  b->stat_count = ramd_dev_alloc(S * sizeof(long long));
  e->d_scratch = ramd_dev_alloc(256 * 16);
  e->d_ranges = ramd_dev_alloc(130 * sizeof(int));
  e->d_dense = ramd_dev_alloc((S + F) * (size_t)RAMD_MAX(s->input_size, s->b_in) * fl);
  if (bI) {
    size_t bn = (size_t)bI * bO;
    b->bw = ramd_dev_alloc(bn * fl);
    b->bm = ramd_dev_alloc(bn * fl);
    b->baux = obl->aux ? ramd_dev_alloc(bn * fl) : NULL;
    b->bdelta = ramd_dev_alloc(bn * fl);
    b->binp = ramd_dev_alloc((S + F) * bI * fl);
    b->bout = ramd_dev_alloc((S + F) * bO * fl);
    b->berr = ramd_dev_alloc(S * bO * fl);
    b->bcarry = ramd_dev_alloc(2 * (size_t)bO * fl);
    b->bcarry_cur = 0;
    b->blast = ramd_dev_alloc(16);
    ramd_h2d(b->blast, obl->inputs + obl->input_size, fl); /* the host's buffer is kept current (set_opinion) */
    ramd_dsync();
  }
  e->lr_pushed = ramd_zalloc(S * sizeof(float));
  e->idx_pushed = ramd_zalloc(S * sizeof(int));
  if (keep_text) {
    b->text = ramd_dev_alloc((size_t)keep_text_len + 1);
    ramd_h2d(b->text, keep_text, (size_t)keep_text_len);
    b->text_len = keep_text_len;
    ramd_dsync();
    free(keep_text);
  }
  if (keep_ext) {
    b->ih_delta = keep_ext;
    b->ho_delta = keep_ext + e->ih_size;
    e->delta_external = 1;
  }
  e->dev_ready = 1;
  e->dev_valid = 0;
  e->err_pending = 0;
  for (int i = 0; i < e->n_streams; i++) {
    ramd_priv(e->streams[i])->dev_valid = 0;
  }
  for (int i = 0; i < e->n_fwd; i++) {
    ramd_priv(e->fwd[i])->dev_valid = 0;
  }
  ramd_dsync();
}

/* The trainers' block buffer (RamdEngine.d_block) has room for `bytes`: synchronised, freed and allocated anew only when
 * it has to grow.  The three block calls share it, which is sound for the reason that one trainer reusing it between two
 * calls is: every upload into it and every launch that reads it is ordered on ramd_stream, so a call's uploads land behind
 * the reads of whichever call used it before; only a free needs the synchronisation (an earlier block's generations may
 * still be reading the old buffer). */
void *ramd_block_room(RamdEngine *e, size_t bytes) {
  ramd_engine_ensure_device(e);
  if (bytes > e->d_block_bytes) {
    ramd_dsync();
    ramd_dev_free(e->d_block);
    e->d_block = ramd_dev_alloc(bytes);
    e->d_block_bytes = bytes;
  }
  return e->d_block;
}
