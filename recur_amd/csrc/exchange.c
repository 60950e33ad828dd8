/* exchange.c -- the exchange step between the ranks of a distributed training set (gnu11 C): the all-reduce
 * overlapped with the weight-delta GEMM (ramd_delta_half_ready; the collective itself is dist.c's), and the exchange
 * as kernel-issued peer traffic -- export, join, leave and the sharded update (include/recur_amd.h).
 */
#define RAMD_HIP_HOST 1
#include "rnn_host.h"
#include <unistd.h>
#include <time.h>

/* The exchange step overlapped with the weight-delta GEMM: the GEMM runs as two
 * row halves (kernels_bptt.hip: g_delta_half_hook); as soon as a half's deltas are complete its sum over the
 * ranks starts on a stream of its own, so the first half's all-reduce (2.2 of the 4.6 MB at the north
 * star) travels over xGMI while the second half is still being multiplied.  The update waits for both.
 * Every rank reduces the same two ranges in the same order, so the replicas stay bit-identical. */
static hipStream_t g_comm_stream = NULL;
static hipEvent_t g_half_ready[2];
hipEvent_t ramd_half_summed[2];
int ramd_halves_seen = 0;

void ramd_delta_half_ready(void *ctx, int half, size_t first_float, size_t n_floats) {
  RamdEngine *e = ctx;
  if (!g_comm_stream) {
    HIP_OK(hipStreamCreateWithFlags(&g_comm_stream, hipStreamNonBlocking));
    ramd_note_side_stream();
    for (int h = 0; h < 2; h++) {
      HIP_OK(hipEventCreateWithFlags(&g_half_ready[h], hipEventDisableTiming));
      HIP_OK(hipEventCreateWithFlags(&ramd_half_summed[h], hipEventDisableTiming));
    }
  }
  HIP_OK(hipEventRecord(g_half_ready[half], ramd_stream));
  HIP_OK(hipStreamWaitEvent(g_comm_stream, g_half_ready[half], 0));
  ramd_dist_all_reduce_on(e->b.ih_delta + first_float, n_floats, g_comm_stream);
  HIP_OK(hipEventRecord(ramd_half_summed[half], g_comm_stream));
  ramd_halves_seen |= 1 << half;
}

/* ---- the exchange step as kernel-issued peer traffic (include/recur_amd.h; kernels_apply.hip: k_apply_xchg) ---- */
typedef struct XchgBlob {
  uint64_t pid;
  uint64_t nonce;     /* of this export: the ranks' blobs together name the session (xchg_session_token) */
  uint64_t raw[3];    /* delta, ih_w, ho_w as this process sees them                        */
  uint64_t offset[3]; /* of each inside its allocation (IPC handles name whole allocations) */
  hipIpcMemHandle_t handle[3];
} XchgBlob;

void rnn_amd_set_exchange_export(RnnAmdSet *set, void *blob) {
  RamdEngine *e = set->eng;
  _Static_assert(sizeof(XchgBlob) <= RNN_AMD_EXCHANGE_BLOB_BYTES, "the blob outgrew its public size");
  ramd_engine_need_dev(e, RNN_AMD_WEIGHTS | RNN_AMD_MOMENTUMS | RNN_AMD_DELTAS);
  ramd_deltas_materialize(e);
  XchgBlob b;
  memset(&b, 0, sizeof(b));
  b.pid = (uint64_t)getpid();
  {
    static uint64_t exports = 0;
    struct timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    b.nonce = ((uint64_t)ts.tv_sec << 30) ^ (uint64_t)ts.tv_nsec ^ (++exports << 48);
    int dev = 0;
    HIP_OK(hipGetDevice(&dev));
    b.nonce = (b.nonce & ~(uint64_t)0xff) | (uint64_t)(dev & 0xff); /* (low byte: the exporting rank's device, for the join's peer-access check) */
  }
  void *arrays[3] = {e->b.ih_delta, e->b.ih_w, e->b.ho_w};
  for (int k = 0; k < 3; k++) {
    hipDeviceptr_t base = NULL;
    size_t size = 0;
    HIP_OK(hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)arrays[k]));
    b.raw[k] = (uint64_t)(uintptr_t)arrays[k];
    b.offset[k] = (uint64_t)((char *)arrays[k] - (char *)base);
    if (hipIpcGetMemHandle(&b.handle[k], (void *)base) != hipSuccess) {
      (void)hipGetLastError(); /* (peers of the same process do not need it) */
      memset(&b.handle[k], 0, sizeof(b.handle[k]));
    }
  }
  memset(blob, 0, RNN_AMD_EXCHANGE_BLOB_BYTES);
  memcpy(blob, &b, sizeof(b));
}

void rnn_amd_set_exchange_leave(RnnAmdSet *set) {
  RamdEngine *e = set->eng;
  if (!e->xchg_world) {
    return;
  }
  ramd_dsync();
  for (int p = 0; p < e->xchg_world; p++) {
    for (int k = 0; k < 3; k++) {
      if (e->xchg_opened[p][k]) {
        (void)hipIpcCloseMemHandle(e->xchg_opened[p][k]);
        e->xchg_opened[p][k] = NULL;
      }
    }
  }
  if (e->xchg_flags_host) {
    (void)hipHostUnregister(e->xchg_flags_host);
  }
  e->xchg_flags_host = NULL;
  e->xchg_flags_dev = NULL;
  e->xchg_world = 0;
}

/* The session's name: every rank holds the same `world` blobs in the same order, every export has its own nonce -- a
 * 32-bit hash of them all is the same on every rank and new for every session.  Even and not 0: T = arrived, T | 1 = has
 * read the counters. */
static unsigned xchg_session_token(const void *blobs, int world) {
  unsigned h = 2166136261u; /* FNV-1a */
  const unsigned char *p = blobs;
  for (size_t i = 0; i < (size_t)world * RNN_AMD_EXCHANGE_BLOB_BYTES; i++) {
    h = (h ^ p[i]) * 16777619u;
  }
  h &= ~1u;
  return h ? h : 2u;
}

/* The join is COLLECTIVE between processes: a rendezvous on the host in words 8 .. 15 of the shared counters (the
 * barrier kernels count in words 0 .. 7).  Phase 1: everybody has arrived in THIS session (stale words of an earlier
 * one do not match its token); then every rank reads where the barrier counters stand; phase 2: everybody has read them
 * -- only then may anyone step and move them.  Bounded: RECUR_AMD_XCHG_JOIN_TIMEOUT seconds (default 120). */
static int xchg_rendezvous(unsigned *c, int rank, int world, unsigned token, unsigned *top_out) {
  const char *te = getenv("RECUR_AMD_XCHG_JOIN_TIMEOUT");
  double limit = te && atof(te) > 0 ? atof(te) : 120.0;
  struct timespec t0, t;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  for (int phase = 0; phase < 2; phase++) {
    if (phase == 1) {
      unsigned top = __atomic_load_n(&c[0], __ATOMIC_ACQUIRE);
      for (int p = 1; p < world; p++) {
        const unsigned v = __atomic_load_n(&c[p], __ATOMIC_ACQUIRE);
        if ((int)(v - top) > 0) {
          top = v;
        }
      }
      *top_out = top;
    }
    __atomic_store_n(&c[8 + rank], token | (unsigned)phase, __ATOMIC_RELEASE);
    for (int p = 0; p < world; p++) {
      for (;;) {
        const unsigned v = __atomic_load_n(&c[8 + p], __ATOMIC_ACQUIRE);
        if (v == (token | 1u) || (phase == 0 && v == token)) {
          break;
        }
        clock_gettime(CLOCK_MONOTONIC, &t);
        if ((t.tv_sec - t0.tv_sec) + 1e-9 * (t.tv_nsec - t0.tv_nsec) > limit) {
          fprintf(stderr, "librecur_amd: rnn_amd_set_exchange_join: rank %d has waited %.0f s for rank %d to join (every "
                          "rank calls the join, with the same blobs and counters that all of them map)\n", rank, limit, p);
          return -1;
        }
        usleep(50);
      }
    }
  }
  return 0;
}

int rnn_amd_set_exchange_join(RnnAmdSet *set, int rank, int world, const void *blobs, void *counters, int lockstep) {
  RamdEngine *e = set->eng;
  ramd_set_need_training(set, "rnn_amd_set_exchange_join");
  if (world < 1 || world > 8 || rank < 0 || rank >= world || !blobs || (!lockstep && !counters) || e->sh.bI ||
      e->xchg_world || e->delta_external) {
    fprintf(stderr, "librecur_amd: rnn_amd_set_exchange_join(rank %d, world %d): 1..8 ranks, every rank's blob, shared "
                    "counters unless in lock step, no bottom layer, no external delta buffer, not joined already\n",
            rank, world);
    return -1;
  }
  ramd_engine_need_dev(e, RNN_AMD_WEIGHTS | RNN_AMD_MOMENTUMS | RNN_AMD_DELTAS);
  ramd_deltas_materialize(e);
  { /* can this rank's kernels reach every peer's device at all?  Asked BEFORE anything is opened: a kernel that stores
     * through a pointer it may not use faults, and a launcher that tries this exchange beside RCCL (bench.py --exchange
     * auto) must get a -1 to fall back on, not a dead rank */
    int mydev = 0;
    HIP_OK(hipGetDevice(&mydev));
    for (int p = 0; p < world; p++) {
      XchgBlob b;
      memcpy(&b, (const char *)blobs + (size_t)p * RNN_AMD_EXCHANGE_BLOB_BYTES, sizeof(b));
      const int peerdev = (int)(b.nonce & 0xff);
      int can = 1;
      if (p != rank && peerdev != mydev && hipDeviceCanAccessPeer(&can, mydev, peerdev) != hipSuccess) {
        (void)hipGetLastError();
        can = 0;
      }
      if (!can) {
        fprintf(stderr, "librecur_amd: rank %d (device %d) has no peer access to rank %d's device %d: the kernel-issued "
                        "exchange needs it (use the RCCL all-reduce)\n", rank, mydev, p, peerdev);
        return -1;
      }
    }
  }
  float **dst[3] = {e->xchg_delta, e->xchg_ihw, e->xchg_how};
  void *own[3] = {e->b.ih_delta, e->b.ih_w, e->b.ho_w};
  memset(e->xchg_opened, 0, sizeof(e->xchg_opened));
  for (int p = 0; p < world; p++) {
    XchgBlob b;
    memcpy(&b, (const char *)blobs + (size_t)p * RNN_AMD_EXCHANGE_BLOB_BYTES, sizeof(b));
    for (int k = 0; k < 3; k++) {
      if (p == rank) {
        dst[k][p] = own[k];
      } else if (b.pid == (uint64_t)getpid()) {
        dst[k][p] = (float *)(uintptr_t)b.raw[k]; /* another set of this process */
      } else {
        void *base = NULL;
        if (hipIpcOpenMemHandle(&base, b.handle[k], hipIpcMemLazyEnablePeerAccess) != hipSuccess) {
          fprintf(stderr, "librecur_amd: rank %d cannot open rank %d's arrays (%s): is there peer access between the "
                          "two GPUs, HSA_ENABLE_IPC_MODE_LEGACY=0 set?\n", rank, p, hipGetErrorString(hipGetLastError()));
          e->xchg_world = p + 1;
          rnn_amd_set_exchange_leave(set);
          return -1;
        }
        e->xchg_opened[p][k] = base;
        dst[k][p] = (float *)((char *)base + b.offset[k]);
      }
    }
  }
  e->xchg_flags_dev = NULL;
  e->xchg_flags_host = NULL;
  if (!lockstep) {
    if (hipHostRegister(counters, 64, hipHostRegisterMapped) != hipSuccess ||
        hipHostGetDevicePointer((void **)&e->xchg_flags_dev, counters, 0) != hipSuccess) {
      fprintf(stderr, "librecur_amd: the shared counters cannot be mapped (%s)\n", hipGetErrorString(hipGetLastError()));
      e->xchg_world = world;
      rnn_amd_set_exchange_leave(set);
      return -1;
    }
    e->xchg_flags_host = counters;
    ramd_note_side_stream(); /* the peers' work runs beside ours where the ranks share a GPU */
  }
  e->xchg_world = world;
  e->xchg_rank = rank;
  e->xchg_lockstep = lockstep;
  /* The barriers count on from where the shared counters stand (round 6; they counted from 0 and trusted the launcher to
   * have zeroed them: on counters left from an earlier session the first barriers would have passed at once).  Every
   * rank reads the same `world` words -- between the two phases of the rendezvous, when nobody can be stepping -- and
   * takes the same start: the furthest of them, compared as the barrier compares (wrap-safe). */
  e->xchg_seq = 0;
  if (!lockstep) {
    unsigned top = 0;
    if (xchg_rendezvous(counters, rank, world, xchg_session_token(blobs, world), &top) != 0) {
      rnn_amd_set_exchange_leave(set);
      return -1;
    }
    e->xchg_seq = top;
  }
  return 0;
}

/* A 64-bit checksum of this replica -- ih_weights || ho_weights (|| ih_momentum || ho_momentum) -- for launchers that
 * want to KNOW that the ranks' replicas stayed identical (include/recur_amd.h).  through_kernel: summed by a kernel on
 * the library's stream, through the caches the path's kernels read through; otherwise over a device-to-host copy (the
 * copy engine reads memory).  The two agree unless something stored into the arrays behind the caches' back. */
uint64_t rnn_amd_set_replica_checksum(RnnAmdSet *set, int with_momentum, int through_kernel) {
  RamdEngine *e = set->eng;
  ramd_engine_need_dev(e, RNN_AMD_WEIGHTS | (with_momentum ? RNN_AMD_MOMENTUMS : 0));
  const float *arrays[4] = {e->b.ih_w, e->b.ho_w, e->b.ih_m, e->b.ho_m};
  const size_t n[4] = {e->ih_size, e->ho_size, e->ih_size, e->ho_size};
  const int n_arrays = with_momentum ? 4 : 2;
  uint64_t sum = 0;
  if (through_kernel) {
    unsigned long long *d = ramd_dev_alloc(sizeof(*d));
    ramd_launch_replica_checksum(ramd_stream, n_arrays, arrays, n, d);
    ramd_d2h(&sum, d, sizeof(sum));
    ramd_dsync();
    ramd_dev_free(d);
    return sum;
  }
  uint64_t first = 0;
  for (int k = 0; k < n_arrays; k++) {
    uint32_t *h = malloc(n[k] * sizeof(uint32_t));
    if (!h) {
      fprintf(stderr, "librecur_amd: rnn_amd_set_replica_checksum: out of memory\n");
      abort();
    }
    ramd_d2h(h, arrays[k], n[k] * sizeof(uint32_t));
    ramd_dsync();
    for (size_t i = 0; i < n[k]; i++) {
      sum += (uint64_t)h[i] * (2 * (first + i) + 1);
    }
    first += n[k];
    free(h);
  }
  return sum;
}

void rnn_amd_set_exchange_range(const RnnAmdSet *set, int which, size_t *first, size_t *count) {
  const RamdEngine *e = set->eng;
  const size_t n4 = (which ? e->ho_size : e->ih_size) / 4;
  const int world = e->xchg_world ? e->xchg_world : 1, rank = e->xchg_world ? e->xchg_rank : 0;
  const size_t lo = n4 * (size_t)rank / world, hi = n4 * (size_t)(rank + 1) / world;
  *first = 4 * lo;
  *count = 4 * (hi - lo);
}

static void xchg_barrier(RamdEngine *e) {
  if (!e->xchg_lockstep) {
    ramd_launch_xchg_barrier(ramd_stream, e->xchg_flags_dev, e->xchg_rank, e->xchg_world, ++e->xchg_seq, ramd_abort_word_dev());
  }
}

void rnn_amd_set_apply_exchange(RnnAmdSet *set, int learning_style, float momentum) {
  RamdEngine *e = set->eng;
  if (!e->xchg_world) {
    fprintf(stderr, "librecur_amd: rnn_amd_set_apply_exchange without rnn_amd_set_exchange_join\n");
    abort();
  }
  ramd_engine_need_dev(e, RNN_AMD_WEIGHTS | RNN_AMD_MOMENTUMS | RNN_AMD_DELTAS);
  ramd_deltas_materialize(e);
  float mw, lr, lr_top;
  const int method = ramd_update_rule(set->nets[0]->bptt, learning_style, momentum, &mw, &lr, &lr_top);
  ramd_check_method_arrays(e, method);
  const int W = e->xchg_world;
  float *w[16];
  const float *d[16];
  for (int p = 0; p < W; p++) { /* segment 0: the top layer, 1: the recurrent layer */
    w[p] = e->xchg_how[p];
    w[W + p] = e->xchg_ihw[p];
    d[p] = e->xchg_delta[p] + e->ih_size;
    d[W + p] = e->xchg_delta[p];
  }
  float *m[2] = {e->b.ho_m, e->b.ih_m}, *aux[2] = {e->b.ho_aux, e->b.ih_aux}, *dout[2] = {e->b.ho_delta, e->b.ih_delta};
  size_t n[2] = {e->ho_size, e->ih_size};
  float rate[2] = {lr_top, lr};
  const int tev = ramd_timing_begin(ramd_stream, RAMD_T_XCHG); /* (the two arrivals and the sharded update: what a rank waits and works for) */
  xchg_barrier(e); /* every rank's local sums are complete (and nobody still multiplies with the old weights) */
  ramd_launch_apply_xchg(ramd_stream, method, e->xchg_rank, W, w, d, m, aux, dout, n, rate, momentum, mw);
  xchg_barrier(e); /* every range of the weights has arrived here */
  ramd_timing_end(ramd_stream, tev);
  ramd_engine_dev_wrote(e, RNN_AMD_WEIGHTS | RNN_AMD_MOMENTUMS | RNN_AMD_DELTAS);
}
