// kernels_chain.hip -- the BPTT chain E_i = E_h . W_ih^T over the D steps (recur-nn.c:338-376) as one translation unit:
// here the development builds' stamp readers, device_view and the launchers (chain_plan.h decides), the kernels in
//   k_chain_steps.h    a launch per step: k_chain_main (32 x 32 tiles), k_chain_wide (64 x 64, big sets)
//   k_chain_persist.h  all steps in one launch, 256 workgroups that wait for one another: k_chain_persist (on k_coop.h)
#include "k_coop.h"
#include "chain_plan.h"
#ifdef PC_STAMPS /* development builds only: stamps of the chain's tail (tools/gpu_chain_stamps.py) */
__device__ unsigned long long g_xc_stamps[32];
#define XC_STAMP(i) do { if (blockIdx.x == 0 && threadIdx.x == ((i) == 10 ? 256 : 0)) g_xc_stamps[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define PRO_STAMP(i, tid) do { if (blockIdx.x == PRO_WG && threadIdx.x == (tid)) g_xc_stamps[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define PRO_STAMP_DEP(i, tid, dep) do { if (blockIdx.x == PRO_WG && threadIdx.x == (tid) && (dep) != 0x7ffffff1) g_xc_stamps[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
/* both clocks: slot i the 100 MHz one, slot i + 1 the shader clock (s_memtime): the clock the chip ran at between two of these */
#define PRO_CLOCKS(i, tid) do { if (blockIdx.x == PRO_WG && threadIdx.x == (tid)) { g_xc_stamps[i] = __builtin_amdgcn_s_memrealtime(); g_xc_stamps[(i) + 1] = __builtin_amdgcn_s_memtime(); } } while (0)
#ifndef PRO_WG
#define PRO_WG 0
#endif
#else
#define PRO_STAMP(i, tid) do { } while (0)
#define PRO_STAMP_DEP(i, tid, dep) do { } while (0)
#define PRO_CLOCKS(i, tid) do { } while (0)
#endif
#include "k_extras.h"
BND_DECL(g_bnd_chain, ramd_bnd_chain_stamps)
#include "k_chain_steps.h"
#include "k_chain_persist.h"

// stores the launch-invariant part of the kernel arguments in device memory (device_view)
__global__ void k_store_view(View v, View *dst) { *dst = v; }

/* the device copy of the View for the kernels that take it by pointer, rewritten only when
 * it changes (the ring position is not part of it: those kernels get it as an argument) */
const View *device_view(hipStream_t st, const View &v) {
  static View *d_view = nullptr;
  static View h_view;
  static bool have = false;
  View cur = v;
  cur.b.uniform_idx = 0;
  /* what changes from call to call and none of those kernels reads (the speculated noise's buffers change places every
   * generation; the flags are per pass): left out, or every generation of a noisy net would rewrite the copy twice
   * (5 us each, seen in the multi-head generation's timeline) */
  cur.b.noise_spec = nullptr;
  cur.b.rng_spec = nullptr;
  cur.b.noise_spec_use = 0;
  cur.b.dense_inputs = 0;
  if (!d_view) HIP_CHECK(hipMalloc(&d_view, sizeof(View)));
  if (!have || memcmp(&cur, &h_view, sizeof(View)) != 0) {
    RAMD_LAUNCH(k_store_view, dim3(1), dim3(1), 0, st, cur, d_view);
    h_view = cur;
    have = true;
  }
  return d_view;
}

#ifdef PC_STAMPS
extern "C" void ramd_chain_stamps(unsigned long long *out) {
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pc_stamps), sizeof(unsigned long long) * 2 * 64 * 8));
}
extern "C" void ramd_chain_tail_stamps(unsigned long long *out) {
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_xc_stamps), sizeof(unsigned long long) * 32));
}
#endif

// chain_plan.h decides; what follows launches what the plan says, each kernel family from one place.

/* the one-launch chain's own device state: its flags and tickets, made at its first launch, and its launch number */
static ChainSync *g_chain_sync = nullptr;
static unsigned g_chain_seq = 0;
static unsigned g_ticket_launches = 0; /* launches that drew tickets: 32 per XCD each */
static void chain_sync_clear(void) {
  if (!g_chain_sync) HIP_CHECK(hipMalloc(&g_chain_sync, sizeof(ChainSync)));
  HIP_CHECK(hipMemset(g_chain_sync, 0, sizeof(ChainSync)));
  g_chain_seq = 0;
  g_ticket_launches = 0;
}

/* one launch of k_chain_persist: its segment and what rides in it */
struct PersistLaunch {
  hipStream_t st;
  const View *d_view;
  int uniform_idx, D;
  ChainSegment s;
  SeatRule seats;
  unsigned seq;
  HoWork hw;
  XcWork xc;
};

template <int ACT, int K, bool ONE, bool PAD, bool XD> static void launch_persist(const PersistLaunch &c) {
  const unsigned tseq = c.seats.mode ? 0u : ++g_ticket_launches; /* (coop_rule.h: coop_seat_mode) */
  raise_lds_limit<k_chain_persist<ACT, K, ONE, PAD, XD>>(pc_lds_bytes(K));
  RAMD_LAUNCH((k_chain_persist<ACT, K, ONE, PAD, XD>), dim3(256), dim3(512), pc_lds_bytes(K), c.st, c.d_view, c.uniform_idx,
              c.s.row0, c.s.nrows, c.D, c.seq, g_chain_sync, ramd_abort_word_dev(), c.s.nvalid, c.s.vlo, c.hw, c.xc, c.seats.mode,
              tseq, c.seats.seats);
}
/* the form that starts each burst under the row stores' drain (chain_plan.h: chain_early_blocks), and how often it ran */
static long g_early_launches = 0;
extern "C" long ramd_chain_early_launches(void) { return g_early_launches; }
template <int ACT> static void launch_persist_early(const PersistLaunch &c) {
  const unsigned tseq = c.seats.mode ? 0u : ++g_ticket_launches;
  raise_lds_limit<k_chain_persist_early<ACT, PC_EARLY>>(pc_lds_bytes(1024));
  RAMD_LAUNCH((k_chain_persist_early<ACT, PC_EARLY>), dim3(256), dim3(512), pc_lds_bytes(1024), c.st, c.d_view, c.uniform_idx,
              c.s.row0, c.s.nrows, c.D, c.seq, g_chain_sync, ramd_abort_word_dev(), c.s.nvalid, c.s.vlo, c.hw, c.xc, c.seats.mode,
              tseq, c.seats.seats);
  g_early_launches++;
}
template <int ACT, int K, bool XD> static void launch_persist_tiles(const PersistLaunch &c) {
  if constexpr (K == 1024 && !XD) /* (the text step's tail only: the dense tail keeps its one kernel) */
    if (c.s.early) return launch_persist_early<ACT>(c);
  if (c.s.pad) launch_persist<ACT, K, true, true, XD>(c);
  else if (c.s.one) launch_persist<ACT, K, true, false, XD>(c);
  else launch_persist<ACT, K, false, false, XD>(c);
}
template <int ACT, int K> static void launch_persist_tail(const PersistLaunch &c) {
  if constexpr (K >= 512) /* the tail for dense inputs */
    if (c.xc.on && c.xc.dense) return launch_persist_tiles<ACT, K, true>(c);
  launch_persist_tiles<ACT, K, false>(c);
}
template <int ACT> static void launch_persist_k(const PersistLaunch &c, int hidden_size) {
  switch (hidden_size) {
  case 1024: return launch_persist_tail<ACT, 1024>(c);
  case 512: return launch_persist_tail<ACT, 512>(c);
  default: return launch_persist_tail<ACT, 256>(c);
  }
}

/* `ho`: a pending request for the top layer's delta rides in this launch (and is marked done when the launch stands) */
static bool launch_chain_persist(hipStream_t st, const View *d_view, const RamdShape *sh, const RamdBuffers *b,
                                 const ChainSegment &s, const SeatRule &seats, HoWork *ho, XcWork *xcp) {
  PersistLaunch c = {st, d_view, b->uniform_idx, sh->D, s, seats, 0u, {}, {}};
  /* RECUR_AMD_CHAIN_CHECK=1 -- for a GPU that is shared, where a co-tenant may take CUs in mid-run: every chain
   * launch is followed by a synchronisation and a look at the abort word.  A launch that gave up is then not fatal:
   * the word is reset, the one-launch chain is switched off for the process and THIS call's chain runs again a
   * launch per step (the one-launch chain reads error plane 0 and writes planes >= 1 only: its input is intact).
   * The extras and the control logic do not ride in a launch that may be discarded (they update per-stream state --
   * min_error_factor, the depth statistics -- that a repeat would update twice).  Costs the host-side pipelining:
   * ~15 us per generation.  RECUR_AMD_CHAIN_TEST_GIVEUP=n (n > 1) implies it and pretends that the n-th launch
   * gave up (tests). */
  const int test_giveup = env_int("RECUR_AMD_CHAIN_TEST_GIVEUP", 0);
  const bool checked = env_int("RECUR_AMD_CHAIN_CHECK", 0) || test_giveup > 1;
  if (xcp && !checked) c.xc = *xcp;
  if (xcp && !c.xc.on) xcp->on = 0; /* (the caller then runs the extras as a launch of their own) */
  if (ho && !ho->done) {
    c.hw = *ho;
    c.hw.workers = s.workers, c.hw.idle_only = s.idle_only;
  }
  if (!g_chain_sync || coop_seq_starts_over(g_chain_seq, COOP_CHAIN_SEQ_LIMIT)) {
    HIP_CHECK(hipStreamSynchronize(st));
    chain_sync_clear();
  }
  c.seq = ++g_chain_seq;
  int ev = timing_begin(st, T_CHAIN, 1);
  if (sh->activation == 2) launch_persist_k<2>(c, sh->hidden_size);
  else if (sh->activation == 5) launch_persist_k<5>(c, sh->hidden_size);
  else launch_persist_k<1>(c, sh->hidden_size);
  timing_end(st, ev);
  if (checked) {
    static int checked_launches = 0;
    HIP_CHECK(hipStreamSynchronize(st));
    const unsigned word = ramd_chain_abort_word();
    if (word || ++checked_launches == test_giveup) {
      fprintf(stderr, "librecur_amd: a one-launch BPTT chain gave up in mid-run (code %u: its 256 workgroups were no longer "
                      "all resident, or a hand-off timed out); this call's chain runs again a launch per step, which is "
                      "what the process uses from here on\n", word);
      coop_mark_broken();
      chain_sync_clear();
      return false;
    }
  }
  if (ho && c.hw.dst) ho->done = 1;
  return true;
}

/* the launch-per-step forms: D launches of one kernel over the call's rows */
struct StepsLaunch {
  hipStream_t st;
  const View *d_view;
  int uniform_idx, row0, nrows, D;
  ChainSteps f;
};
template <int NS, int MT> static void launch_wide_steps(const StepsLaunch &c) {
  const size_t shm = (size_t)W_STAGES * W_STAGE_FLOATS * sizeof(float);
  raise_lds_limit<k_chain_wide<NS, MT>>((int)shm);
  for (int t = 0; t < c.D; t++)
    RAMD_LAUNCH((k_chain_wide<NS, MT>), dim3(c.f.blocks), dim3(512), shm, c.st, c.d_view, c.uniform_idx, c.row0, c.nrows, t,
                c.f.tm, c.f.tn);
}
template <int NS> static void launch_wide_mt(const StepsLaunch &c) {
  if (c.f.mt == 32) launch_wide_steps<NS, 32>(c);
  else launch_wide_steps<NS, 64>(c);
}
template <bool UNI, int NS> static void launch_main_steps(const StepsLaunch &c) {
  for (int t = 0; t < c.D; t++)
    RAMD_LAUNCH((k_chain_main<UNI, NS>), dim3(c.f.blocks), dim3(512), 0, c.st, c.d_view, c.uniform_idx, c.row0, c.nrows, t,
                c.f.tm, c.f.tn, c.f.nstages);
}
static void launch_chain_steps(const StepsLaunch &c) {
  /* one event pair around the D launches: the per-launch average then carries
   * 1/D of the event overhead instead of all of it */
  int ev = timing_begin(c.st, T_CHAIN, c.D);
  const int ns = c.f.ns;
  if (c.f.form == CHAIN_WIDE) {
    if (ns == 32) launch_wide_mt<32>(c);
    else if (ns == 24) launch_wide_mt<24>(c);
    else launch_wide_mt<16>(c);
  } else if (!c.f.uniform) launch_main_steps<false, 0>(c);
  else if (ns == 16) launch_main_steps<true, 16>(c);
  else if (ns == 8) launch_main_steps<true, 8>(c);
  else if (ns == 4) launch_main_steps<true, 4>(c);
  else if (ns == 2) launch_main_steps<true, 2>(c);
  else launch_main_steps<true, 0>(c);
  timing_end(c.st, ev);
}

/* All D steps of the chain for streams [row0, row0 + nrows) (the part of rnn_bptt_calc_deltas between the
 * top layer's backprop and the extras): the one-launch chain where it applies, otherwise a launch per
 * step with 64 x 64 or 32 x 32 tiles.  Returns the partial sums of squares per (step, stream) it left. */
int ramd_chain_steps(hipStream_t st, const View &v, const RamdShape *sh, const RamdBuffers *b, int row0,
                     int nrows, HoWork *ho, XcWork *xc) {
  const View *d_view = device_view(st, v);
  /* (the probe behind the seats is a launch and a wait, once: only a call that wants the one-launch chain asks) */
  const SeatRule seats = chain_persist_wanted(sh, b, row0, nrows) ? coop_seat_rule(st) : SeatRule{};
  const ChainPlan p = ramd_plan_chain(sh, b, row0, nrows, seats.resident);
  bool persist = p.seg_rows > 0;
  ChainSegment s;
  /* (RECUR_AMD_CHAIN_CHECK: a launch that gave up ends them; all of the call's rows go through the steps below) */
  for (int r = 0; persist && chain_segment(p, r, &s); r += s.nrows) persist = launch_chain_persist(st, d_view, sh, b, s, seats, ho, xc);
  if (!persist) {
    launch_chain_steps(StepsLaunch{st, d_view, b->uniform_idx, row0, nrows, sh->D, p.steps});
    return p.steps.tn_parts;
  }
  if (xc && xc->on) xc->done = 1; /* every launch of the chain carried its rows' extras and control */
  return 0; /* the one-launch chain leaves no partial sums: the extras sum the rows themselves */
}
