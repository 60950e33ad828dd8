// kernels_forward.hip -- rnn_bptt_advance and rnn_opinion on the device: the launchers of the forward pass.  The kernels:
// k_fwd_stages.h (history advance, input assembly, bottom layer, presynaptic noise, the finishing kernels), the hidden
// layer's forms in k_fwd_wide.h, k_fwd_fused.h, k_fwd_top.h, k_fwd_small.h (and k_gemm.h), the output layer in k_fwd_out.h.
#include "k_gemm.h"
#include "fwd_plan.h"
#include "k_fwd_stages.h"
#include "k_fwd_wide.h"
#include "k_fwd_fused.h"
#include "k_fwd_top.h"
#include "k_fwd_small.h"
#include "k_fwd_out.h"

// ------------------------------------------------- the pass: plan, then a short function per stage --
// fwd_plan.h decides; what follows launches what the plan says, each kernel from one place.

template <int NS>
static void launch_fwd_wide_ns(hipStream_t st, const View *d_view, const RamdBuffers *b, int row0, int nrows, const FwdTiles &t,
                               const WideOp &op) {
  const size_t shm = (size_t)W_STAGES * W_STAGE_FLOATS * sizeof(float);
  raise_lds_limit<k_fwd_wide<NS>>((int)shm);
  RAMD_LAUNCH(k_fwd_wide<NS>, dim3(t.blocks), dim3(512), shm, st, d_view, b->uniform_idx, row0, nrows, t.tm, t.tn, op);
}
/* op.a == nullptr: the hidden layer's operands, from the View */
static void launch_fwd_wide(hipStream_t st, const View &v, const RamdBuffers *b, int row0, int nrows, const FwdTiles &t,
                            const WideOp &op, int cls) {
  const View *d_view = device_view(st, v);
  int ev = timing_begin(st, cls);
  if (t.ns == 33) launch_fwd_wide_ns<33>(st, d_view, b, row0, nrows, t, op);
  else if (t.ns == 17) launch_fwd_wide_ns<17>(st, d_view, b, row0, nrows, t, op);
  else launch_fwd_wide_ns<9>(st, d_view, b, row0, nrows, t, op);
  timing_end(st, ev);
}

template <int NS>
static void launch_fwd_fused_ns(hipStream_t st, const View *d_view, const RamdBuffers *b, const RamdFwdCall *c, const FwdPlan &p) {
  RAMD_LAUNCH((k_fwd_fused<NS>), dim3(p.ht.blocks), dim3(512), 0, st, d_view, b->uniform_idx, c->row0, c->nrows, p.ht.tm,
              p.ht.tn, p.nstages, c->mode, c->text_i, c->global_first, c->global_count, c->dense, c->ld);
}

/* the text step's pass and its top layer as one launch, where fwd_top_plan.h says so; false: nothing launched */
static FwdTopSync *g_ft_sync = nullptr;
static unsigned g_ft_seq = 0;
static long g_ft_launches = 0;
static bool launch_fwd_top(hipStream_t st, const View &v, const RamdShape *sh, const RamdBuffers *b, const RamdFwdCall *c,
                           const FwdPlan &p) {
  if (!fwd_top_shape_ok(sh, b, c, p)) return false; /* (first: the probe behind the seats is a launch and a wait, once) */
  const SeatRule sr = coop_seat_rule(st);
  if (!fwd_top_seats_ok(sr)) return false;
  if (!g_ft_sync) {
    HIP_CHECK(hipMalloc(&g_ft_sync, sizeof(FwdTopSync)));
    HIP_CHECK(hipMemset(g_ft_sync, 0, sizeof(FwdTopSync)));
  }
  if (coop_seq_starts_over(g_ft_seq, COOP_FWD_TOP_SEQ_LIMIT)) {
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipMemset(g_ft_sync, 0, sizeof(FwdTopSync)));
    g_ft_seq = 0;
  }
  const View *d_view = device_view(st, v);
  int ev = timing_begin(st, T_FWD);
  RAMD_LAUNCH(k_fwd_top<8>, dim3(256), dim3(1024), 0, st, d_view, b->uniform_idx, c->row0, c->nrows, c->text_i, c->global_first,
              c->global_count, g_ft_sync, ++g_ft_seq, ramd_abort_word_dev(), sr.seats);
  timing_end(st, ev);
  g_ft_launches++;
  return true;
}
extern "C" long ramd_fwd_top_launches(void) { return g_ft_launches; }

static void stage_input(hipStream_t st, const View &v, const RamdShape *sh, const RamdFwdCall *c, const FwdPlan &p) {
  if (p.input == FIN_BOTTOM) {
    if (p.advance_first) RAMD_LAUNCH(k_advance, dim3((c->nrows + 255) / 256), dim3(256), 0, st, v, c->row0, c->nrows);
    RAMD_LAUNCH(k_bottom_forward, dim3(c->nrows), dim3(256), (size_t)(sh->bI + sh->bO) * sizeof(float), st, v, c->row0,
                c->mode, c->dense, c->ld, c->text_i, c->global_first, c->global_count, c->noise);
  }
  if (p.input == FIN_BOTTOM || p.input == FIN_ASSEMBLE) {
    const bool keep = p.input == FIN_BOTTOM; /* the layer's outputs are the real inputs, and the ring has stepped */
    RAMD_LAUNCH(k_assemble, dim3(c->nrows), dim3(256), 0, st, v, c->row0, keep ? (int)RAMD_IN_KEEP : c->mode,
                keep ? nullptr : c->dense, keep ? 0 : c->ld, keep ? 0 : c->text_i, c->global_first, c->global_count,
                keep ? 0 : c->advance);
  }
}

static void stage_hidden(hipStream_t st, const View &v, const RamdBuffers *b, const RamdFwdCall *c, const FwdPlan &p) {
  const int row0 = c->row0, nrows = c->nrows;
  if (p.hidden == FH_SMALL) {
    int ev = timing_begin(st, T_FWD);
    RAMD_LAUNCH(k_fwd_small, dim3(1), dim3(1024), 0, st, v, row0);
    timing_end(st, ev);
  } else if (p.hidden == FH_FUSED) {
    const View *d_view = device_view(st, v);
    int ev = timing_begin(st, T_FWD);
    if (p.ht.ns == 8) launch_fwd_fused_ns<8>(st, d_view, b, c, p);
    else if (p.ht.ns == 4) launch_fwd_fused_ns<4>(st, d_view, b, c, p);
    else if (p.ht.ns == 2) launch_fwd_fused_ns<2>(st, d_view, b, c, p);
    else if (p.ht.ns == 16) launch_fwd_fused_ns<16>(st, d_view, b, c, p);
    else launch_fwd_fused_ns<0>(st, d_view, b, c, p);
    timing_end(st, ev);
  } else if (p.hidden == FH_WIDE) {
    launch_fwd_wide(st, v, b, row0, nrows, p.ht, WideOp{}, T_FWD);
  } else if (p.uniform) {
    ProbFwd<true> pr = {v, row0, nrows};
    launch_gemm<false, true, ProbFwd<true>>(st, pr, b->slab, nrows, v.sh.H, p.nkt, p.ks, T_FWD);
  } else {
    ProbFwd<false> pr = {v, row0, nrows};
    launch_gemm<false, true, ProbFwd<false>>(st, pr, b->slab, nrows, v.sh.H, p.nkt, p.ks, T_FWD);
  }
}

/* (behind k_fwd_fused the values generated ahead are added by its finishing kernel: stage_hidden_end) */
static void stage_noise(hipStream_t st, const View &v, const RamdFwdCall *c, const FwdPlan &p) {
  if (p.hidden == FH_FUSED) return;
  if (p.noise == FN_APPLY)
    RAMD_LAUNCH(k_noise_apply, dim3((c->nrows * (v.sh.H / 4) + 255) / 256), dim3(256), 0, st, v, c->row0, c->nrows);
  else if (p.noise == FN_GENERATE)
    RAMD_LAUNCH(k_presynaptic_noise, dim3((c->nrows + 63) / 64), dim3(64), 0, st, v, c->row0, c->nrows, c->noise);
}

static void stage_hidden_end(hipStream_t st, const View &v, const RamdFwdCall *c, const FwdPlan &p) {
  const int nrows = c->nrows;
  if (p.end == FE_FINALIZE) {
    RAMD_LAUNCH(k_fwd_finalize, dim3((nrows * (v.sh.H / 4) + 255) / 256), dim3(256), 0, st, v, c->row0, nrows, p.ks);
  } else if (p.end == FE_FINALIZE_FUSED) { /* the sums' tail columns, the noise generated ahead, the activation */
    const int nmain = (nrows * (v.sh.H / 4 - 1) + 255) / 256;
    RAMD_LAUNCH(k_fwd_finalize_fused, dim3(nmain + (nrows + 7) / 8), dim3(256), 0, st, v, c->row0, nrows, p.ht.tn,
                p.noise == FN_APPLY, nmain);
  }
}

static void stage_output(hipStream_t st, const View &v, const RamdShape *sh, const RamdBuffers *b, const RamdFwdCall *c,
                         const FwdPlan &p) {
  const int row0 = c->row0, nrows = c->nrows;
  if (p.output == FO_O4) {
    RAMD_LAUNCH(k_out_layer_o4, dim3((nrows + 3) / 4), dim3(256), 0, st, v, row0, nrows);
  } else if (p.output == FO_ROWS) {
    RAMD_LAUNCH(k_out_layer, dim3(nrows), dim3(1024), (size_t)(sh->H + OUT_SEGS * 64) * sizeof(float), st, v, row0);
  } else if (p.output == FO_WIDE) {
    WideOp op = {b->hidden + (size_t)row0 * sh->H, b->ho_w, b->out + (size_t)row0 * sh->O, sh->H, sh->O, sh->O, sh->H, sh->O};
    launch_fwd_wide(st, v, b, row0, nrows, p.ot, op, T_OTHER);
  } else if (p.output == FO_GEMM) {
    ProbOut pr = {v, row0, nrows};
    launch_gemm<false, true, ProbOut>(st, pr, b->slab, nrows, sh->O, p.o_nkt, p.o_ks, T_OTHER);
    RAMD_LAUNCH(k_sum_slabs, dim3((nrows * (sh->O / 4) + 255) / 256), dim3(256), 0, st, b->out + (size_t)row0 * sh->O, sh->O,
                b->slab, nrows, sh->O, p.o_ks, 0);
  }
}

extern "C" RamdHandover ramd_launch_forward(ramd_stream_t st_, const RamdShape *sh, const RamdBuffers *b, const RamdFwdCall *c,
                                            void (*seam)(void *ctx), void *ctx) {
  hipStream_t st = (hipStream_t)st_;
  View v = make_view(sh, b);
  const FwdPlan p = ramd_plan_forward(sh, b, c);
  if (launch_fwd_top(st, v, sh, b, c, p)) return RamdHandover{0, 0, 1}; /* the top layer is done too */
  stage_input(st, v, sh, c, p);
  stage_hidden(st, v, b, c, p);
  stage_noise(st, v, c, p);
  stage_hidden_end(st, v, c, p);
  if (seam && p.end == FE_FINALIZE_FUSED) seam(ctx);
  stage_output(st, v, sh, b, c, p);
  return p.left;
}

extern "C" void ramd_launch_noise_speculate(ramd_stream_t st_, const RamdShape *sh, const RamdBuffers *b,
                                            int row0, int nrows, float noise, float *out_noise, void *out_states,
                                            const void *src_states, const int *loss_classes, int n_classes, int skip) {
  hipStream_t st = (hipStream_t)st_;
  View v = make_view(sh, b);
  RAMD_LAUNCH(k_noise_speculate, dim3((nrows + 63) / 64), dim3(64), 0, st, v, row0, nrows, noise, out_noise,
              (DevRng *)out_states, (const DevRng *)src_states, loss_classes, n_classes, skip);
}
