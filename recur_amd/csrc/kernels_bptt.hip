// kernels_bptt.hip -- the rest of rnn_bptt_calc_deltas (the chain itself: kernels_chain.hip) as one translation unit:
// ramd_launch_calc_deltas, a pure plan (calc_plan.h) and one short function per stage, and the stages' kernels in the
// headers included below, in pipeline order:
//   k_bptt_top.h      the top layer backwards and its weight delta
//   k_bptt_extras.h   extras + control behind the chain (on k_extras.h)
//   k_delta_direct.h  the weight-delta GEMM without a K split (k_delta_direct_ho, which needs View, is here beside it)
//   k_delta_dma.h     the weight-delta GEMM by LDS-DMA (the generic forms: k_gemm.h)
//   k_bptt_small.h    the one-workgroup form of all of it for one stream of a small net
// Here: the bottom layer's two kernels, the finalizes (k_delta_finalize, k_err_writeback, k_zero_f4) and every launcher.
#include "k_common.h"
#include "k_gemm.h"
#include "calc_plan.h"

// cumulative_input_error of one stream (recur-nn.c:377-382): the input columns of
// every executed step's error, summed in step order.  One workgroup per stream.
__global__ __launch_bounds__(64) void k_bottom_error(View v, int row0, int nxp,
                                                     const unsigned char *active) {
  const RamdShape &s = v.sh;
  int j = blockIdx.x, r = row0 + j;
  int n = (active && !active[j]) ? 0 : v.b.n_exec[r];
  for (int y = threadIdx.x; y < s.bO; y += 64) {
    float sum = 0.0f;
    if (y < s.input_size)
      for (int k = 0; k < n; k++) sum += v.b.ex[((size_t)(k + 1) * s.Scap + r) * nxp + y + 1];
    v.b.berr[(size_t)r * s.bO + y] = sum;
  }
}

// single_layer_sgd on the bottom layer (recur-nn.c:750-757, 256-273) for the streams in
// the reference's order.  bottom->o_error is shared by all the clones and only
// rnn_bptt_clear_deltas ever zeroes it, so stream j's update uses the running total of
// every stream before it (and of every earlier generation): carry_in + the prefix sum.
// One thread per weight; the stream loop is sequential, as the reference's calls are.
__global__ __launch_bounds__(256) void k_bottom_delta(View v, int row0, int nrows, int accumulate,
                                                      const unsigned char *active,
                                                      const float *carry_in, float *carry_out) {
  const RamdShape &s = v.sh;
  int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= s.bI * s.bO) return;
  int yi = e / s.bO, x = e - yi * s.bO;
  float cum = carry_in[x];
  float acc = accumulate ? v.b.bdelta[e] : 0.0f;
  for (int j = 0; j < nrows; j++) {
    if (active && !active[j]) continue;
    int r = row0 + j;
    cum += v.b.berr[(size_t)r * s.bO + x];
    /* a stream whose error gain was clipped shrinks the accumulator -- all of it, it is the layer's
     * one o_error -- by ih_scale twice (recur-nn.c:391-399); an unclipped stream has ih_scale 1 */
    const float sc = v.b.ih_scale[r];
    if (sc != 1.0f && x < s.input_size) cum *= sc * sc;
    float xi = v.b.binp[(size_t)r * s.bI + yi];
    if (xi != 0.0f) acc += xi * cum;
  }
  v.b.bdelta[e] = acc;
  if (yi == 0) carry_out[x] = cum;
}

#include "k_bptt_top.h"
#include "k_bptt_extras.h"

BND_DECL(g_bnd_delta, ramd_bnd_delta_stamps)
#ifdef BND_STAMPS
#define DD_BND_MARK(which) BND_MARK(g_bnd_delta, which)
#endif
#include "k_delta_direct.h" /* the weight-delta GEMM without a K split over workgroups (hidden 1024 and up) */

#ifdef PC_STAMPS
extern "C" void ramd_ddir_stamps(unsigned long long *out) {
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ddir_stamps), sizeof(unsigned long long) * 32));
  HIP_CHECK(hipMemcpyFromSymbol(out + 32, HIP_SYMBOL(g_ddir_wave), sizeof(unsigned long long) * 32));
}
extern "C" void ramd_ddir_clocks(unsigned long long *out) {
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ddir_clk), sizeof(unsigned long long) * 16));
}
#endif
/* k_delta_direct with the top layer's weight delta AND its update in the launch's first microseconds (the fused text step):
 * workgroup i forms rows 5 i .. of ho_delta = hidden^T . o_error over the call's streams (chain_ho_delta, k_common.h: what
 * the chain launch otherwise does in ITS first 2.5 us, on the generation's critical path), stores them and updates those
 * rows of W_ho and its momentum (recur-nn.c:482-487 with the top layer's rate, 653-676) -- between the request for the
 * GEMM's first operands and the first wait for them (dd_body's PRE): the waves of this launch wait ~2 us there anyway. */
template <int NW, int P, int NPW>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(NW / 4, NW / 4))) void k_delta_direct_ho(DdArgs a, View v,
                                                                                                                HoWork hw, HoApply ap) {
  extern __shared__ __attribute__((aligned(16))) float ddh_lds[];
  __builtin_amdgcn_s_setprio(2);
  BND_MARK(g_bnd_delta, 0);
#ifndef DD_HO_AT_END
#define DD_HO_AT_END 1
#endif
#if DD_HO_AT_END /* round 6 (profiles/NOTES_r06.md): the hook behind the GEMM's epilogue instead of in front of its first wait */
  dd_body<NW, P, NPW>(a, ddh_lds);
  __syncthreads();
  chain_ho_delta<5, 8>(v, hw, ddh_lds, (int)blockIdx.x, ap);
#else
  dd_body<NW, P, NPW>(a, ddh_lds, [&]() { chain_ho_delta<5, 8>(v, hw, ddh_lds, (int)blockIdx.x, ap); });
#endif
  BND_MARK(g_bnd_delta, 1);
}

#include "k_delta_dma.h"
#include "k_bptt_small.h"

// ------------------------------------------------------- finalize: delta --

// ih_delta (+)= sum of the K slabs (recur-nn.c:735-748 folded: the per-stream
// ih_scale already multiplies the error rows that went into the GEMM)
__global__ __launch_bounds__(256) void k_delta_finalize(float *delta, const float *slab,
                                                        size_t n4, size_t n, int ks,
                                                        int accumulate, int H, int hidden_size,
                                                        int rows_core, int ks_rest,
                                                        const float *rest, size_t rest_stride,
                                                        float *ho_delta, const float *ho_slab,
                                                        size_t ho_n, int ho_ks) {
  size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t ih_threads = ((n4 + 255) / 256) * 256;
  if (q >= ih_threads) {
    /* the blocks past ih_delta: ho_delta (+)= its K slabs, when the caller has them pending
     * (k_ho_delta_finalize without error ranges) */
    size_t e = q - ih_threads;
    if (ho_slab && 4 * e < ho_n) {
      float4 a = accumulate ? ld4(ho_delta + 4 * e) : zero4();
      for (int z = 0; z < ho_ks; z++) {
        float4 t = ld4(ho_slab + (size_t)z * ho_n + 4 * e);
        a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
      }
      *reinterpret_cast<float4 *>(ho_delta + 4 * e) = a;
    }
    return;
  }
  if (q >= n4) return;
  /* rows below rows_core were produced with ks K slices, the others with ks_rest (their own planes) */
  const float *src = slab + 4 * q;
  size_t stride = n;
  if ((int)((4 * q) / (size_t)H) >= rows_core) {
    ks = ks_rest;
    src = rest + (4 * q - (size_t)rows_core * H);
    stride = rest_stride;
  }
  float4 a = accumulate ? ld4(delta + 4 * q) : zero4();
  float4 sum = sum_planes(src, stride, ks);
  /* the GEMM only produced columns 1..hidden_size; the others are exactly zero */
  int c = (int)((4 * q) % (size_t)H);
  a.x += (c + 0 >= 1 && c + 0 <= hidden_size) ? sum.x : 0.0f;
  a.y += (c + 1 >= 1 && c + 1 <= hidden_size) ? sum.y : 0.0f;
  a.z += (c + 2 >= 1 && c + 2 <= hidden_size) ? sum.z : 0.0f;
  a.w += (c + 3 >= 1 && c + 3 <= hidden_size) ? sum.w : 0.0f;
  *reinterpret_cast<float4 *>(delta + 4 * q) = a;
}

extern "C" void ramd_launch_pending_finalize(ramd_stream_t st_, const RamdPendingDelta *p) {
  hipStream_t st = (hipStream_t)st_;
  const size_t n4 = p->slab ? p->n / 4 : 0;
  const unsigned blocks = (unsigned)((n4 + 255) / 256) + (p->ho_slab ? (unsigned)((p->ho_n / 4 + 255) / 256) : 0u);
  if (!blocks) return;
  RAMD_LAUNCH(k_delta_finalize, dim3(blocks), dim3(256), 0, st, p->delta_out, p->slab, n4, p->n, p->ks, 0, p->H,
              p->hidden_size, p->rows_core, p->ks_rest, p->rest, p->rest_stride, p->ho_delta_out, p->ho_slab, p->ho_n,
              p->ho_ks);
}

// Rebuilds bptt->h_error (err_a) and bptt->i_error (err_b) as the reference leaves them (write_error_images,
// k_common.h), one workgroup per stream.
__global__ __launch_bounds__(256) void k_err_writeback(View v, int row0, int nxp) {
  int r = row0 + blockIdx.x;
  int n = v.b.n_exec[r];
  if (n <= 0) return;
  for (int i = threadIdx.x; i < v.sh.I; i += 256) write_error_images(v, r, n, nxp, i);
}

__global__ void k_zero_f4(float *a, size_t n4) {
  size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < n4) *reinterpret_cast<float4 *>(a + 4 * q) = zero4();
}

extern "C" void ramd_launch_bottom_deltas(ramd_stream_t st_, const RamdShape *sh, RamdBuffers *b,
                                          int row0, int nrows, int accumulate,
                                          const unsigned char *active) {
  hipStream_t st = (hipStream_t)st_;
  View v = make_view(sh, b);
  RAMD_LAUNCH(k_bottom_error, dim3(nrows), dim3(64), 0, st, v, row0, ramd_nxp(sh), active);
  int n = sh->bI * sh->bO;
  const float *cin = b->bcarry + (size_t)b->bcarry_cur * sh->bO;
  float *cout = b->bcarry + (size_t)(b->bcarry_cur ^ 1) * sh->bO;
  RAMD_LAUNCH(k_bottom_delta, dim3((n + 255) / 256), dim3(256), 0, st, v, row0, nrows,
                     accumulate, active, cin, cout);
  b->bcarry_cur ^= 1;
}

extern "C" void ramd_launch_clear_deltas(ramd_stream_t st_, const RamdShape *sh,
                                         const RamdBuffers *b) {
  hipStream_t st = (hipStream_t)st_;
  size_t ih4 = (size_t)sh->I * sh->H / 4, ho4 = (size_t)sh->H * sh->O / 4;
  RAMD_LAUNCH(k_zero_f4, dim3((unsigned)((ih4 + 255) / 256)), dim3(256), 0, st, b->ih_delta, ih4);
  RAMD_LAUNCH(k_zero_f4, dim3((unsigned)((ho4 + 255) / 256)), dim3(256), 0, st, b->ho_delta, ho4);
  if (sh->bI) { /* recur-nn.c:687-692 */
    size_t b4 = (size_t)sh->bI * sh->bO / 4, c4 = (size_t)2 * sh->bO / 4;
    RAMD_LAUNCH(k_zero_f4, dim3((unsigned)((b4 + 255) / 256)), dim3(256), 0, st, b->bdelta, b4);
    RAMD_LAUNCH(k_zero_f4, dim3((unsigned)((c4 + 255) / 256)), dim3(256), 0, st, b->bcarry, c4);
  }
}

static int g_calc_wrote_images = 0;
/* Multi-GPU: the weight-delta GEMM in two row halves, so that the sum over the ranks of the first half
 * can travel while the second half is still being multiplied (set_train.c sets the hook for the call it
 * wants split; the launcher calls it after each half's deltas are complete in ih_delta || ho_delta,
 * with the half's range in floats from ih_delta). */
static void (*g_delta_half_hook)(void *ctx, int half, size_t first_float, size_t n_floats) = nullptr;
static void *g_delta_half_ctx = nullptr;
extern "C" void ramd_set_delta_half_hook(void (*hook)(void *, int, size_t, size_t), void *ctx) {
  g_delta_half_hook = hook;
  g_delta_half_ctx = ctx;
}
/* whether the last ramd_launch_calc_deltas also rebuilt bptt->h_error / i_error (reads and clears) */
extern "C" int ramd_calc_wrote_images(void) {
  int w = g_calc_wrote_images;
  g_calc_wrote_images = 0;
  return w;
}

/* One call of ramd_launch_calc_deltas: its arguments, the kernels' view of the buffers, and the plan (calc_plan.h). */
struct CalcCall {
  hipStream_t st;
  View v;
  const RamdShape *sh;
  const RamdBuffers *b; /* (from the weight deltas on, with the caller's workspace as its slab: CalcPlan::own_ws) */
  int row0, nrows, accumulate;
  const int *ranges;
  int range_stride;
  const unsigned char *active;
  RamdPendingDelta *defer;
  CalcPlan p;
};

static void calc_top_backprop(const CalcCall &c) {
  const RamdShape *sh = c.sh;
  const RamdBuffers *b = c.b;
  const CalcPlan &p = c.p;
  if (p.writeback_first) ramd_launch_err_writeback(c.st, sh, b, c.row0, c.nrows); /* the images, before anything below overwrites the planes */
  const size_t shm = (size_t)(sh->O + sh->H) * sizeof(float);
  if (p.top == TOP_SPARSE) {
    /* the multi-head loss's ranges, only the heads a stream trained: partial products per (stream, head), then the
     * ordered sums and the clip */
    const int alen = b->mheads_alen, ncls = sh->output_size / alen;
    const int span4 = (3 + alen + 3) / 4, ld = (4 * span4) | 1; /* (the widest span: a head that starts 3 columns into its float4) */
    raise_lds_limit<k_top_heads_partial>(96 * 1024); /* (85 KB at 128 symbols) */
    RAMD_LAUNCH(k_top_heads_partial, dim3(ncls, (sh->H + THP_ROWS - 1) / THP_ROWS), dim3(256),
                (size_t)((THP_ROWS + 32) * ld + 4) * sizeof(float), c.st, c.v, c.row0, c.nrows, c.ranges, c.range_stride, c.active,
                alen, ncls, b->mheads_part);
    RAMD_LAUNCH(k_top_heads_combine, dim3(c.nrows), dim3(THC_THREADS), 0, c.st, c.v, c.row0, c.ranges, c.range_stride, c.active,
                ncls, b->mheads_part, (p.flags & RAMD_IMAGES_PENDING) ? 1 : 0); /* (it takes the stale entries from the planes) */
  } else if (p.top == TOP_HEADS) {
    /* the multi-head loss's ranges: one GEMM over all streams (k_top_backprop_heads), then the sums and the clip */
    const int tm = (c.nrows + 31) / 32, tn = (sh->H + 31) / 32;
    RAMD_LAUNCH(k_top_backprop_heads, dim3(tm * tn), dim3(512), (size_t)((sh->O + 15) / 16) * sizeof(unsigned), c.st, c.v,
                c.row0, c.nrows, c.ranges, c.range_stride, c.active, b->slab, p.top_nb, tm);
    RAMD_LAUNCH(k_top_backprop_scale, dim3(c.nrows), dim3(256), 0, c.st, c.v, c.row0, c.active, b->slab, p.top_nb);
  } else if (p.top == TOP_RANGED) {
    RAMD_LAUNCH(k_top_backprop_ranged, dim3(c.nrows, p.top_nb), dim3(1024), shm, c.st, c.v, c.row0, c.ranges, c.range_stride,
                c.active, b->slab);
    if (p.top_nb > 1) RAMD_LAUNCH(k_top_backprop_scale, dim3(c.nrows), dim3(256), 0, c.st, c.v, c.row0, c.active, b->slab, p.top_nb);
  } else if (p.top == TOP_PLAIN)
    RAMD_LAUNCH(k_top_backprop, dim3(c.nrows), dim3(256), shm, c.st, c.v, c.row0, c.ranges, c.range_stride, c.active);
}

/* What the top layer's delta still owes after its stage: a split-K GEMM into b->ho_slab that waits for a launch of the
 * weight-delta stage to share, and whether its planes are summed in this call (sum_here) or by the optimiser launch
 * that follows (defer->ho_*). */
struct HoOwed {
  bool gemm, sum_here;
  ProbHoDelta prob;
  int nkt, ks;
};

/* The top layer's delta, unless k_delta_direct forms it (ho_in_delta) or the fused single-net path updates W_ho
 * directly (RAMD_NO_HO_DELTA).  Called in front of the chain launch -- which takes it as a request where the plan
 * asks (req) -- and, where it was asked, again with the chain's answer: the GEMM when the chain declined. */
static HoOwed calc_top_delta(const CalcCall &c, HoWork *req, bool chain_answered) {
  const RamdShape *sh = c.sh;
  const RamdBuffers *b = c.b;
  RamdPendingDelta *defer = c.defer;
  HoOwed owed = {};
  if (c.p.ho_in_delta || (c.p.flags & RAMD_NO_HO_DELTA)) return owed;
  if (c.p.ho_asked && !chain_answered) {
    req->dst = (defer && b->ho_slab) ? b->ho_slab : b->ho_delta;
    req->active = c.active;
    req->row0 = c.row0;
    req->nrows = c.nrows;
    return owed;
  }
  if (c.p.ho_asked && req->done) {
    if (defer) { /* one plane for the optimiser launch to take (or ho_delta is complete already) */
      defer->ho_slab = req->dst == b->ho_slab ? b->ho_slab : nullptr;
      defer->ho_n = (size_t)sh->H * sh->O;
      defer->ho_ks = 1;
      defer->ho_delta_out = b->ho_delta;
    }
    return owed;
  }
  const HoGemmPlan h = ramd_plan_ho_gemm(sh, b, c.p, c.nrows, c.accumulate, c.ranges != nullptr, c.range_stride,
                                         c.active != nullptr, defer != nullptr);
  if (defer) defer->ho_slab = nullptr;
  if (h.form == HO_HEADS) { /* only the heads a stream trained carry error */
    const int alen = b->mheads_alen, ncls = sh->output_size / alen;
    RAMD_LAUNCH(k_ho_delta_heads, dim3(ncls, (sh->H + 31) / 32), dim3(256), (size_t)(HDH_K * ((alen | 1) + 32) + 8) * sizeof(float),
                c.st, c.v, c.row0, c.nrows, c.ranges, c.range_stride, c.active, alen, ncls, c.accumulate);
    return owed;
  }
  /* per-stream 1.0 / 0.0 participation flags as floats (b->coef plane 0 is free here:
   * k_bptt_control rewrites it later in this call) */
  const float *live = b->ones + c.row0;
  if (c.active) {
    RAMD_LAUNCH(k_live_mask, dim3((c.nrows + 255) / 256), dim3(256), 0, c.st, b->coef + c.row0, c.active, c.nrows);
    live = b->coef + c.row0;
  }
  const ProbHoDelta prob = {c.v, c.row0, c.nrows, live};
  if (h.form == HO_PLANES_PAIRED || h.form == HO_PAIRED_SUMMED)
    owed = {true, h.form == HO_PAIRED_SUMMED, prob, h.nkt, h.ks};
  else
    launch_gemm<true, true, ProbHoDelta>(c.st, prob, h.form == HO_PLANES ? b->ho_slab : b->slab, sh->H, sh->O, h.nkt, h.ks, T_OTHER);
  if (h.form == HO_PLANES || h.form == HO_PLANES_PAIRED) {
    defer->ho_slab = b->ho_slab;
    defer->ho_n = (size_t)sh->H * sh->O;
    defer->ho_ks = h.ks;
    defer->ho_delta_out = b->ho_delta;
  }
  if (h.form == HO_SUMMED)
    /* with one range list per stream the set of touched columns differs per stream; the
     * error is zero outside a stream's own ranges, so every column may take its sum */
    RAMD_LAUNCH(k_ho_delta_finalize, dim3((sh->H * sh->O + 255) / 256), dim3(256), 0, c.st, c.v, b->slab, h.ks, c.accumulate,
                c.range_stride ? nullptr : c.ranges);
  return owed;
}

/* The owed top-layer GEMM (launch_it; the pair launch has launched it already) and, where its planes are summed in
 * this call, their sum -- unless the k_delta_finalize that ends the call may take it along (may_ride): returns that. */
static bool calc_settle_owed(const CalcCall &c, HoOwed &owed, bool launch_it, bool may_ride) {
  if (!owed.gemm) return false;
  if (launch_it) launch_gemm<true, true, ProbHoDelta>(c.st, owed.prob, c.b->ho_slab, c.sh->H, c.sh->O, owed.nkt, owed.ks, T_OTHER);
  owed.gemm = false;
  if (!owed.sum_here) return false;
  if (may_ride && !c.ranges) return true;
  RAMD_LAUNCH(k_ho_delta_finalize, dim3((c.sh->H * c.sh->O + 255) / 256), dim3(256), 0, c.st, c.v, c.b->ho_slab, owed.ks,
              c.accumulate, c.range_stride ? nullptr : c.ranges);
  return false;
}

/* one stream of a small net: chain, extras, control and weight deltas in one workgroup */
static void calc_small(const CalcCall &c) {
  raise_lds_limit<k_bptt_small>(150 * 1024);
  if (c.defer) c.defer->slab = nullptr; /* ih_delta is written here: nothing left for the optimiser to sum */
  int ev = timing_begin(c.st, T_CHAIN, 1);
  RAMD_LAUNCH(k_bptt_small, dim3(1), dim3(1024), c.p.small_lds, c.st, c.v, c.row0, c.accumulate, c.p.flags, c.p.nx, c.p.nxp);
  timing_end(c.st, ev);
  g_calc_wrote_images = 1; /* the error images are done: no k_err_writeback for this call */
}

/* the extras and the control logic as a request to the one-launch chain's tail */
static XcWork calc_xc_request(const CalcCall &c) {
  XcWork xc = {};
  if (c.p.xc_req == XC_NONE) return xc;
  xc.on = 1;
  xc.dense = c.p.xc_req == XC_DENSE;
  xc.row0 = c.row0;
  xc.nx = c.p.nx;
  xc.nxp = c.p.nxp;
  xc.active = c.active;
  xc.flags = c.p.flags;
  return xc;
}

/* ... and where the chain declined (tn_parts: the partial sums of squares per (step, stream) it left) */
static void calc_extras_control(const CalcCall &c, int tn_parts) {
  const RamdShape *sh = c.sh;
  const CalcPlan &p = c.p;
  const size_t shm = (size_t)(2 * sh->D + 1) * sizeof(float);
  if (p.extras == XF_CONTROL5) /* extras and control in one launch, one workgroup per stream */
    RAMD_LAUNCH((k_extras_control<5, 1024>), dim3(c.nrows), dim3(1024), shm, c.st, c.v, c.row0, c.nrows, p.nx, p.nxp, tn_parts,
                c.active, p.flags);
  else if (p.extras == XF_CONTROL8)
    RAMD_LAUNCH((k_extras_control<8, 512>), dim3(c.nrows), dim3(512), shm, c.st, c.v, c.row0, c.nrows, p.nx, p.nxp, tn_parts,
                c.active, p.flags);
  else if (p.extras == XF_CONTROL9)
    RAMD_LAUNCH((k_extras_control<9, 512>), dim3(c.nrows), dim3(512), shm, c.st, c.v, c.row0, c.nrows, p.nx, p.nxp, tn_parts,
                c.active, p.flags);
  else if (p.extras == XF_DENSE)
    ramd_launch_extras_dense(c.st, c.v, sh, c.row0, c.nrows, p.nx, p.nxp, tn_parts, 0, sh->D);
  else {
    const int M = sh->D * c.nrows;
    ProbExtras prob = {c.v, c.row0, c.nrows, p.nx};
    launch_gemm<false, false, ProbExtras>(c.st, prob, c.b->slab, M, p.nxp, (sh->H + BK - 1) / BK, p.xks, T_OTHER);
    RAMD_LAUNCH(k_extras_finalize, dim3(M), dim3(64), 0, c.st, c.v, c.row0, c.nrows, p.nx, p.nxp, p.xks, tn_parts);
  }
  if (p.extras == XF_DENSE || p.extras == XF_GEMM)
    RAMD_LAUNCH(k_bptt_control, dim3((c.nrows + 3) / 4), dim3(256), 0, c.st, c.v, c.row0, c.nrows, c.active, p.flags, p.tn);
}

/* What a weight-delta GEMM left in the workspace for the optimiser launch, or k_delta_finalize, to sum: ks planes of
 * the rows below rows_core and ks_rest planes of the rows from there on. */
struct DeltaPlanes {
  int ks, rows_core, ks_rest;
  const float *rest; /* plane z of the rest rows: rest + z * rest_stride */
  size_t rest_stride;
  bool ho_rides; /* the owed top-layer planes are summed along with them */
};
/* whole planes, every row of ih_delta in each of the ks (ks_rest: the rest is empty, nobody reads it) */
static DeltaPlanes whole_planes(const CalcCall &c, int ks, int ks_rest) {
  return {ks, c.sh->I, ks_rest, c.b->slab + c.p.n, c.p.n, false};
}

static void launch_delta_finalize(const CalcCall &c, size_t first, size_t floats, int ks, int rows_core, int ks_rest, const float *rest,
                                  size_t rest_stride, const float *ho_slab, size_t ho_n, int ho_ks) {
  const size_t n4 = floats / 4;
  const unsigned blocks = (unsigned)((n4 + 255) / 256) + (ho_slab ? (unsigned)(((size_t)c.sh->H * c.sh->O / 4 + 255) / 256) : 0u);
  RAMD_LAUNCH(k_delta_finalize, dim3(blocks), dim3(256), 0, c.st, c.b->ih_delta + first, c.b->slab + first, n4, c.p.n, ks,
              c.accumulate, c.sh->H, c.sh->hidden_size, rows_core, ks_rest, rest, rest_stride, c.b->ho_delta, ho_slab, ho_n, ho_ks);
}

template <int NPW> static void launch_delta_direct(const CalcCall &c, const DdArgs &a, const HoWork *hw, const HoApply *ap) {
  const int tiles = c.p.dtm * c.p.dtn;
  if (hw) {
    raise_lds_limit<k_delta_direct_ho<DNW, DP, NPW>>(dd_lds_bytes(DNW, NPW));
    RAMD_LAUNCH((k_delta_direct_ho<DNW, DP, NPW>), dim3(tiles), dim3(64 * DNW), dd_lds_bytes(DNW, NPW), c.st, a, c.v, *hw, *ap);
  } else {
    raise_lds_limit<k_delta_direct<DNW, DP, NPW>>(dd_lds_bytes(DNW, NPW));
    RAMD_LAUNCH((k_delta_direct<DNW, DP, NPW>), dim3(c.p.dks * tiles), dim3(64 * DNW), dd_lds_bytes(DNW, NPW), c.st, a);
  }
}

/* k_delta_direct (k_delta_direct.h): 64 x 64 tiles that own ALL of K, where those fill the chip (hidden 1024: 256 tiles);
 * the sum goes straight into ih_delta -- and, when the caller's update is the momentum rule and nothing else wants the
 * sums first, weights and momentum are updated in the same epilogue (fuse_want).  Returns whether the call is complete
 * (no K split); else *out are the planes. */
static bool calc_delta_direct(const CalcCall &c, HoOwed &owed, DeltaPlanes *out) {
  const RamdShape *sh = c.sh;
  const RamdBuffers *b = c.b;
  const CalcPlan &p = c.p;
  RamdPendingDelta *defer = c.defer;
  calc_settle_owed(c, owed, true, false);
  /* the top layer's sum as ONE array by now?  (the chain launch formed it, or a finalize has run) */
  const bool ho_planes = defer && defer->ho_slab; /* (planes of a split-K GEMM: the epilogue adds them) */
  const float *ho_src = ho_planes ? defer->ho_slab : b->ho_delta;
  const bool fuse = p.direct_fuse && (ho_src || p.ho_in_delta);
  DdArgs a = {};
  a.x = b->arena + (size_t)c.row0 * sh->I;
  a.e = b->ehi + (size_t)c.row0 * sh->I + 1;
  a.coef = b->coef + c.row0;
  a.n_exec = b->n_exec + c.row0;
  a.ih_scale = b->ih_scale + c.row0;
  a.w = b->ih_w + 1;
  a.m = b->ih_m + 1;
  a.delta = b->ih_delta + 1;
  a.plane = (size_t)sh->Scap * sh->I;
  a.I = sh->I;
  a.H = sh->H;
  a.Scap = sh->Scap;
  a.nrows = c.nrows;
  a.D = sh->D;
  a.uidx = b->uniform_idx;
  a.tm = p.dtm;
  a.tn = p.dtn;
  a.rest = p.drest;
  a.rgroups = p.drg;
  a.fast_its = p.fast_its;
  a.hidden_size = sh->hidden_size;
  a.mode = fuse ? 2 : c.accumulate ? 1 : 0;
  if (p.dks > 1) { /* planes: stored, summed (and added to ih_delta where the call accumulates) by what follows */
    a.delta = b->slab + 1;
    a.ksplit = p.dks;
    a.kplane = p.n;
    a.mode = 0;
  }
  if (fuse) {
    a.rate = defer->fuse_rate;
    a.momentum = defer->fuse_momentum;
    a.mw = defer->fuse_mw;
    a.method = defer->fuse_method;
    if (!p.ho_in_delta) { /* the top layer's sums are there (the chain launch formed them): its update, shared out */
      a.ho_w = b->ho_w;
      a.ho_m = b->ho_m;
      a.ho_delta = ho_src;
      a.ho_delta_out = ho_src == b->ho_delta ? nullptr : b->ho_delta;
      a.ho_ks = ho_planes ? defer->ho_ks : 1;
      a.ho_plane = defer->ho_n;
      a.ho_n4 = (unsigned)((size_t)sh->H * sh->O / 4);
      a.ho_rate = defer->fuse_ho_rate;
    }
  }
  /* ... or formed HERE, in the launch's first microseconds (its waves wait ~2 us for their first operands anyway):
   * workgroup i sums and updates rows 5 i .. of ho_delta / W_ho / its momentum -- 2.5 us less in the chain launch */
  const bool ho_here = fuse && p.ho_in_delta;
  HoWork hw = {};
  hw.dst = b->ho_delta;
  hw.row0 = c.row0;
  hw.nrows = c.nrows;
  hw.workers = p.dtm * p.dtn;
  const HoApply ap = ho_here ? HoApply{b->ho_w, b->ho_m, defer->fuse_ho_rate, defer->fuse_momentum, defer->fuse_mw} : HoApply{};
  int ev = timing_begin(c.st, T_DELTA);
  if (p.npw == 2)
    launch_delta_direct<2>(c, a, ho_here ? &hw : nullptr, &ap);
  else
    launch_delta_direct<1>(c, a, ho_here ? &hw : nullptr, &ap);
  timing_end(c.st, ev);
  if (p.dks > 1) {
    *out = whole_planes(c, p.dks, p.ks);
    return false;
  }
  if (defer) {
    defer->slab = nullptr; /* ih_delta is complete */
    if (fuse) {
      defer->ho_slab = nullptr;
      defer->fuse_done = 1;
    }
  }
  return true;
}

/* rest: its rest rows (DeltaRest) ride along, their planes d.rest_off floats into the workspace */
static void launch_delta_dma(const CalcCall &c, const GemmOut &o, int blocks, const DmaPlan &d, bool rest) {
  const size_t shm = (size_t)DD_STAGES * DD_STAGE_FLOATS * sizeof(float), shm_rest = shm + (size_t)DD_REST_FLOATS * sizeof(float);
  DeltaRest dr = {};
  if (rest) dr = {c.b->slab + d.rest_off, d.rest_plane, d.rest_rows, d.rows_core};
  if (!rest) {
    raise_lds_limit<k_delta_dma<0>>((int)shm);
    RAMD_LAUNCH(k_delta_dma<0>, dim3(blocks), dim3(512), shm, c.st, c.v, c.row0, c.nrows, o, dr);
  } else if (d.rest_rows <= 64) {
    raise_lds_limit<k_delta_dma<64>>((int)shm_rest);
    RAMD_LAUNCH(k_delta_dma<64>, dim3(blocks), dim3(512), shm_rest, c.st, c.v, c.row0, c.nrows, o, dr);
  } else {
    raise_lds_limit<k_delta_dma<128>>((int)shm_rest);
    RAMD_LAUNCH(k_delta_dma<128>, dim3(blocks), dim3(512), shm_rest, c.st, c.v, c.row0, c.nrows, o, dr);
  }
}

/* The two-halves form (see g_delta_half_hook): rows [0, tm / 2 tiles), summed into ih_delta, hook; then the upper tiles
 * with the rest rows riding along, the top layer's deltas (ho_direct: complete since the chain launch), summed, hook. */
static void calc_delta_dma_halves(const CalcCall &c, const DmaPlan &d, GemmOut o, const HoOwed &owed, bool ho_direct) {
  const RamdShape *sh = c.sh;
  const size_t half_floats = (size_t)d.tmh * 128 * sh->H, up_floats = c.p.n - half_floats, ho_n = (size_t)sh->H * sh->O;
  o.tm = d.tmh;
  o.ks = d.kd2;
  int ev = timing_begin(c.st, T_DELTA, 2);
  launch_delta_dma(c, o, d.blocks2, d, false); /* lower half: no rest rows */
  launch_delta_finalize(c, 0, half_floats, d.kd2, d.tmh * 128, 0, c.b->slab, 0, nullptr, 0, 0);
  g_delta_half_hook(g_delta_half_ctx, 0, 0, half_floats);
  o.row0m = d.tmh * 128; /* upper half + rest rows + the top layer */
  launch_delta_dma(c, o, d.blocks2, d, true);
  timing_end(c.st, ev);
  if (!ho_direct) launch_gemm<true, true, ProbHoDelta>(c.st, owed.prob, c.b->ho_slab, sh->H, sh->O, owed.nkt, owed.ks, T_OTHER);
  launch_delta_finalize(c, half_floats, up_floats, d.kd2, d.rows_core - d.tmh * 128, d.kd2 * d.tmh, c.b->slab + d.rest_off,
                        d.rest_plane, ho_direct ? nullptr : c.b->ho_slab, ho_direct ? 0 : ho_n, ho_direct ? 0 : owed.ks);
  g_delta_half_hook(g_delta_half_ctx, 1, half_floats, up_floats + ho_n);
}

/* k_delta_dma: whole 128-row tiles by LDS-DMA, one workgroup per CU; the rows above them (the input rows of a text
 * net) inside the launch, or by the generic kernel with its own K split -- one launch with the owed top-layer GEMM.
 * Returns whether the call is complete (the two halves); else *out are the planes. */
static bool calc_delta_dma(const CalcCall &c, HoOwed &owed, bool ho_direct, DeltaPlanes *out) {
  const RamdShape *sh = c.sh;
  const RamdBuffers *b = c.b;
  const CalcPlan &p = c.p;
  const DmaPlan d = ramd_plan_delta_dma(sh, p, c.ranges != nullptr, c.defer != nullptr, g_delta_half_hook != nullptr,
                                        (owed.gemm && owed.sum_here) || ho_direct);
  const int ncol = sh->hidden_size + 1;
  GemmOut o;
  o.slab = b->slab;
  o.M = sh->I;
  o.N = ncol;
  o.ldc = sh->H;
  o.zs = p.n;
  o.nkt = p.nkt;
  o.tm = d.tm;
  o.tn = d.tn;
  o.ks = d.kd;
  o.col0 = 1;
  o.row0m = 0;
  if (d.halves) {
    calc_delta_dma_halves(c, d, o, owed, ho_direct);
    return true;
  }
  int ev = timing_begin(c.st, T_DELTA);
  launch_delta_dma(c, o, d.blocks, d, d.rest_in);
  timing_end(c.st, ev);
  *out = {d.kd, d.rows_core, d.ks_rest, d.ks_rest ? b->slab + d.rest_off : b->slab + (size_t)d.rows_core * sh->H,
          d.ks_rest ? d.rest_plane : p.n, false};
  if (d.rest_in) {
    out->ho_rides = calc_settle_owed(c, owed, true, true);
  } else if (d.rest_rows > 0) {
    ProbDelta<true> prob = {c.v, c.row0, c.nrows, p.rtiles};
    float *rest_slab = b->slab + d.rest_off - (size_t)d.rows_core * sh->H; /* (row rows_core of its planes is their first) */
    if (owed.gemm) {
      int blocks_a, blocks_b;
      GemmOut oa = make_gemm_out(b->ho_slab, sh->H, sh->O, owed.nkt, owed.ks, 0, 0, 0, &blocks_a);
      GemmOut ob = make_gemm_out(rest_slab, sh->I, ncol, p.nkt, d.ks_rest, 1, sh->H, d.rows_core, &blocks_b);
      ob.zs = d.rest_plane;
      int ev2 = timing_begin(c.st, T_DELTA);
      RAMD_LAUNCH((k_gemm_pair<ProbHoDelta, ProbDelta<true>>), dim3(blocks_a + blocks_b), dim3(256), 0, c.st, owed.prob, oa,
                  blocks_a, prob, ob);
      timing_end(c.st, ev2);
      out->ho_rides = calc_settle_owed(c, owed, false, true);
    } else {
      launch_gemm<true, true, ProbDelta<true>>(c.st, prob, rest_slab, sh->I, ncol, p.nkt, d.ks_rest, T_DELTA, 1, sh->H,
                                               d.rows_core, d.rest_plane);
    }
  }
  return false;
}

/* the generic GEMMs: 128 x 128 tiles where there are enough of them */
static DeltaPlanes calc_delta_generic(const CalcCall &c) {
  const RamdShape *sh = c.sh;
  const CalcPlan &p = c.p;
  const int ncol = sh->hidden_size + 1;
  if (c.b->uniform_idx >= 0) {
    ProbDelta<true> prob = {c.v, c.row0, c.nrows, p.rtiles};
    if (p.big)
      launch_gemm2<ProbDelta<true>>(c.st, prob, c.b->slab, sh->I, ncol, p.nkt, p.ks, T_DELTA, 1, sh->H);
    else
      launch_gemm<true, true, ProbDelta<true>>(c.st, prob, c.b->slab, sh->I, ncol, p.nkt, p.ks, T_DELTA, 1, sh->H);
  } else {
    ProbDelta<false> prob = {c.v, c.row0, c.nrows, p.rtiles};
    if (p.big)
      launch_gemm2<ProbDelta<false>>(c.st, prob, c.b->slab, sh->I, ncol, p.nkt, p.ks, T_DELTA, 1, sh->H);
    else
      launch_gemm<true, true, ProbDelta<false>>(c.st, prob, c.b->slab, sh->I, ncol, p.nkt, p.ks, T_DELTA, 1, sh->H);
  }
  return whole_planes(c, p.ks, p.ks);
}

/* the planes go to the optimiser launch that follows, which sums the slabs itself, or are summed here */
static void calc_hand_over(const CalcCall &c, const DeltaPlanes &d, const HoOwed &owed) {
  RamdPendingDelta *defer = c.defer;
  if (defer && !c.accumulate) {
    defer->slab = c.b->slab;
    defer->n = c.p.n;
    defer->ks = d.ks;
    defer->H = c.sh->H;
    defer->hidden_size = c.sh->hidden_size;
    defer->rows_core = d.rows_core;
    defer->ks_rest = d.ks_rest;
    defer->rest = d.rest;
    defer->rest_stride = d.rest_stride;
    defer->delta_out = c.b->ih_delta;
    return;
  }
  if (defer) defer->slab = nullptr;
  launch_delta_finalize(c, 0, c.p.n, d.ks, d.rows_core, d.ks_rest, d.rest, d.rest_stride, d.ho_rides ? c.b->ho_slab : nullptr,
                        (size_t)c.sh->H * c.sh->O, owed.ks);
}

extern "C" void ramd_launch_calc_deltas(ramd_stream_t st_, const RamdShape *sh,
                                        const RamdBuffers *b, int row0, int nrows, int accumulate,
                                        const int *ranges, int range_stride,
                                        const unsigned char *active, unsigned flags,
                                        RamdPendingDelta *defer) {
  g_calc_wrote_images = 0;
  CalcCall c = {(hipStream_t)st_, make_view(sh, b), sh, b, row0, nrows, accumulate, ranges, range_stride, active, defer,
                ramd_plan_calc_deltas(sh, b, row0, nrows, accumulate, ranges != nullptr, range_stride, active != nullptr, flags,
                                      defer, g_delta_half_hook != nullptr)};
  calc_top_backprop(c);
  HoWork ho_req = {};
  HoOwed owed = calc_top_delta(c, &ho_req, false);
  if (c.p.small) return calc_small(c);
  // BPTT chain: D dependent steps, then the extras of all steps and the control logic -- in its tail, or behind it
  XcWork xc_req = calc_xc_request(c);
  const int tn_parts = ramd_chain_steps(c.st, c.v, sh, b, row0, nrows, c.p.ho_asked ? &ho_req : nullptr, xc_req.on ? &xc_req : nullptr);
  if (c.p.ho_asked) owed = calc_top_delta(c, &ho_req, true);
  if (!xc_req.done) calc_extras_control(c, tn_parts);
  // weight deltas: one GEMM over (step, stream)
  RamdBuffers own_ws;
  if (c.p.own_ws) { /* (the kernels' View, made above, is not concerned: the planes reach them as arguments) */
    own_ws = *b;
    own_ws.slab = defer->own_slab;
    own_ws.slab_floats = defer->own_slab_floats;
    c.b = &own_ws;
  }
  const bool ho_direct = c.p.ho_asked && ho_req.done && ho_req.dst == b->ho_delta; /* complete since the chain launch */
  DeltaPlanes planes = {};
  bool complete = false;
  if (c.p.direct_runs)
    complete = calc_delta_direct(c, owed, &planes);
  else if (c.p.dma)
    complete = calc_delta_dma(c, owed, ho_direct, &planes);
  else
    planes = calc_delta_generic(c);
  if (!complete) calc_hand_over(c, planes, owed);
}

extern "C" void ramd_launch_err_writeback(ramd_stream_t st_, const RamdShape *sh,
                                          const RamdBuffers *b, int row0, int nrows) {
  hipStream_t st = (hipStream_t)st_;
  View v = make_view(sh, b);
  RAMD_LAUNCH(k_err_writeback, dim3(nrows), dim3(256), 0, st, v, row0, ramd_nxp(sh));
}
