// kernels_loss.hip -- the callers' loss functions on the device (text, multi-text, classify, rnnca) and their launchers.
#include "k_common.h"

// -------------------------------------------------------- loss on device --

#ifdef PC_STAMPS /* development builds only (tools/mkabl.sh -DPC_STAMPS, tools/gpu_top_stamps.py) */
__device__ unsigned long long g_tt_stamps[16];
#define TT_STAMP(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) g_tt_stamps[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define TT_STAMP(i) do { } while (0)
#endif
#include "k_top.h"
#include "k_text_top2.h"
#include "fwd_plan.h"
#include "fwd_top_plan.h"
#include "parrot_rule.h"
#include "sigmoid_rule.h"
#include "classify_train_rule.h"
BND_DECL(g_bnd_top, ramd_bnd_top_stamps)
#pragma clang fp contract(off)

// net_error_bptt's loss (charmodel-predict.c:18-27): softmax (badmaths.h:71-111),
// best guess and negation (badmaths.h:113-141), +1 on the target; plus the
// running statistics of the epoch loop (charmodel-predict.c:302-304).  One
// thread per stream walks its row in the reference's order, so the sums round
// the same way.
__global__ __launch_bounds__(64) void k_softmax_error(View v, int row0, int nrows) {
  extern __shared__ float ex[]; /* [output_size] exponentials */
  int j = blockIdx.x;
  if (j >= nrows) return;
  const RamdShape &s = v.sh;
  int r = row0 + j;
  // zero fraction of the hidden row (recur-nn.c:438-442), counted by the wave
  const float *hid = v.b.hidden + (size_t)r * s.H;
  int zeros = 0;
  for (int i = threadIdx.x; i < s.H; i += 64) zeros += (hid[i] == 0.0f);
  for (int off = 32; off > 0; off >>= 1) zeros += __shfl_down(zeros, off, 64);
  const float *src = v.b.out + (size_t)r * s.O;
  float *err = v.b.o_error + (size_t)r * s.O;
  int len = s.output_size;
  // max and min are order independent: one pass over the lanes; the exponentials in parallel, their sum in the
  // reference's order
  wave_softmax_exps(src, ex, len, threadIdx.x, FenceBlock{});
  // every lane adds the exponentials in the reference's order (the same value in all of
  // them); the divisions and the arg max (first of equal maxima, badmaths.h:126-139) are
  // spread over the lanes
  const float sum = ordered_sum(ex, len);
  BestGuess best;
  const int target = v.b.target[r];
  for (int i = threadIdx.x; i < len; i += 64) {
    float e = ex[i] / sum;
    err[i] = softmax_error(e, i == target);
    best.offer(e, i);
  }
  wave_best_guess(best);
  if (threadIdx.x != 0) return;
  float e = softmax_error(ex[target] / sum, true);
  float l = 1.0f - e;
  v.b.stat_err[r] += e;
  v.b.stat_ent[r] += capped_log2f_dev(l);
  v.b.stat_correct[r] += (best.i == target);
  v.b.stat_count[r] += 1;
  v.b.stat_zero[r] += zeros / (double)s.hidden_size;
}
// The top of a text generation in one launch, one workgroup (16 waves) per stream: the
// output layer (k_out_layer), the softmax loss against the stream's target
// (k_softmax_error) and the top-layer backprop with its soft clip (k_top_backprop, dense
// form), each exactly as in the separate kernels -- same operation order per value -- with
// the hidden row, the outputs and the output error passed through LDS instead of HBM.
#ifdef PC_STAMPS
extern "C" void ramd_top_stamps(unsigned long long *out) {
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tt_stamps), sizeof(unsigned long long) * 16));
}
#endif
/* KIND (RamdTopLoss.kind, ramd_internal.h): which loss sits between the output layer and the backprop -- 0: the text model's
 * softmax against the stream's next symbol; 1: rnnca's sigmoid + squared error (sigmoid_rule.h, gstrnnca.c:701-714); 2:
 * gstclassify's class groups (k_grouped_softmax_error's, gstclassify.c:2070-2119); 3: parrot's tanh + slope error
 * (parrot_rule.h, gstparrot.c:464-477).  1 and 3 serve the dense losses' opinion-plus-loss calls, 2 the class groups':
 * finalize + output layer + loss + top backprop of a dense-input generation in ONE launch instead of four (7.4 + 12.0 + 4.9 +
 * 9.8 us at 2048 / 512, 5.0 + 4.7 + 4.8 + 5.0 us at 512 / 128).  1 and 2 are one wave's work (o_size <= 64); 3 gives every
 * column a thread of its own (o_size <= 256: parrot's 256 bins, waves 0 .. 3). */
struct FastExpDev { /* the rules' exponential on the device */
  __device__ __forceinline__ float operator()(float x) const { return fast_expf_dev(x); }
};
/* The progress figure of the dense losses (parrot_loss, sigmoid_loss), per stream-generation: a row's terms are added up by
 * wave reductions (thread x brings columns x, x + 256, ...), then the waves' sums in order 0 .. 3, and the row's sum and one
 * count go into the set's statistics.  The order is the library's own: the figure is held to a float64 restatement, not bit
 * for bit. */
__device__ __forceinline__ float loss_wave_sum(float term) {
  for (int off = 32; off > 0; off >>= 1) term += __shfl_down(term, off, 64);
  return term;
}
__device__ __forceinline__ float loss_four_waves(const float *wsum) { return ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]; }
__device__ __forceinline__ void loss_add_stats(const View &v, int r, float sum) {
  v.b.stat_err[r] += (double)sum;
  v.b.stat_count[r] += 1;
}
template <int KIND>
__global__ __launch_bounds__(1024) void k_text_top(View v, int row0, int nrows, int fwd_ks, RamdTopLoss tl) {
  extern __shared__ float tsh[];
  __shared__ float tred[16];
  __shared__ float tstat[4];
  __shared__ int trained_sh;
  const RamdShape &s = v.sh;
  const int r = row0 + blockIdx.x;
  float *shid = tsh;                   /* [H] hidden row                    */
  float *part = shid + s.H;            /* [OUT_SEGS][64] float4 of partial sums (16-byte aligned: h_size % 4 == 0) */
  float *sout = part + OUT_SEGS * 64 * 4 + OUT_SEGS * s.O; /* [O] outputs (behind the waves' column sums [OUT_SEGS][O]) */
  float *sex = sout + s.O;             /* [O] exponentials                   */
  float *serr = sex + s.O;             /* [O] output error                   */
  const int seg = threadIdx.x >> 6, lane = threadIdx.x & 63;
  TT_STAMP(0);
  BND_MARK(g_bnd_top, 0);
  /* What does not depend on anything computed here is requested FIRST (round 3, from stamps of the 12.2 us
   * between the first and the last instruction: the target, the pad of o_error and the statistics'
   * read-modify-writes were three memory round trips inside the one-wave softmax): wave 0 asks for the
   * stream's target and the o_error pad here; the statistics are added to by wave 1 behind the softmax's
   * barrier, beside the backprop.  (The output layer's weights too would be wanted here -- 2 us behind the
   * first barrier -- but 14 float4 per lane beside the hidden row's sums do not fit 128 registers, and a
   * spilled prefetch waits for its data on the spot: 258 against 246 us per generation.) */
  const bool wide = (s.O >> 2) <= 64;
  const int OQ = s.O >> 2, RPW = wide ? min(64 / OQ, 8) : 1, rsub = lane / (wide ? OQ : 64), c4 = lane - rsub * OQ;
  const bool rows_mine = wide && rsub < RPW;
  const int per = (s.H + OUT_SEGS - 1) / OUT_SEGS;
  const int y0 = seg * per, y1 = min(s.H, y0 + per);
  constexpr int NB = 14; /* float4 in flight per lane and batch: 66 rows of a wave at 5 rows per instruction */
  int target = 0;
  float pad_oe = 0.0f, mse_target = 0.0f;
  if constexpr (KIND == 3) { /* column x is thread x's: its target and its o_error pad */
    if ((int)threadIdx.x < s.O) {
      pad_oe = v.b.o_error[(size_t)r * s.O + threadIdx.x];
      mse_target = (int)threadIdx.x < tl.n ? tl.targets[(size_t)blockIdx.x * tl.ld + threadIdx.x] : 0.0f;
    }
  } else if (seg == 0) {
    if constexpr (KIND == 0) target = v.b.target[r];
    const int pi = lane < s.O ? lane : 0; /* (o_size > 64: the later columns are read where they are used) */
    pad_oe = v.b.o_error[(size_t)r * s.O + pi];
    if constexpr (KIND == 1) mse_target = lane < tl.n ? tl.targets[(size_t)blockIdx.x * tl.ld + lane] : 0.0f;
  }
  top_hidden_row(v, r, nrows, fwd_ks, shid, WaveSumShfl{});
  __syncthreads();
  TT_STAMP(1);
  // ---- output layer (recur-nn.c:150-151)
  if (wide) {
    /* Rows of W_ho as float4: a wave instruction fetches RPW whole rows (11 lanes x 16 bytes each at o_size 44)
     * instead of one float per lane of one row -- the texture path takes a wave instruction at a time, and
     * 1056 of them per workgroup for 180 KB were 5 us of this kernel.  Lane (rsub, c4) sums rows y0 + rsub,
     * + RPW, ... of its four columns; the RPW x 16 partial sums of a column are added in a fixed order. */
    float4 acc = zero4();
    for (int yb = y0; yb < y1; yb += NB * RPW) {
      float4 wv[NB];
#pragma unroll
      for (int i = 0; i < NB; i++) {
        const int y = yb + rsub + RPW * i;
        wv[i] = ld4(v.b.ho_w + (size_t)((rows_mine && y < y1) ? y : y0) * s.O + 4 * c4);
      }
#pragma unroll
      for (int i = 0; i < NB; i++) {
        const int y = yb + rsub + RPW * i;
        if (rows_mine && y < y1) {
          const float hv = shid[y];
          acc.x += hv * wv[i].x;
          acc.y += hv * wv[i].y;
          acc.z += hv * wv[i].z;
          acc.w += hv * wv[i].w;
        }
      }
    }
    *reinterpret_cast<float4 *>(part + 4 * (seg * 64 + lane)) = acc;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); /* one wave: its own LDS writes are ordered */
    /* the wave's RPW partial sums of a column, rows ascending; then (behind the barrier) the sixteen waves' */
    float *wsum = part + 4 * OUT_SEGS * 64; /* [OUT_SEGS][o_size] */
    for (int col = lane; col < s.O; col += 64) {
      const float *p = part + 4 * (seg * 64 + (col >> 2)) + (col & 3);
      float t[8];
#pragma unroll
      for (int rs = 0; rs < 8; rs++) t[rs] = p[4 * ((rs < RPW ? rs : 0) * OQ)];
      float sum = t[0];
#pragma unroll
      for (int rs = 1; rs < 8; rs++)
        if (rs < RPW) sum += t[rs];
      wsum[seg * s.O + col] = sum;
    }
    __syncthreads();
    if ((int)threadIdx.x < s.O) {
      const int col = threadIdx.x;
      float t[OUT_SEGS];
#pragma unroll
      for (int g = 0; g < OUT_SEGS; g++) t[g] = wsum[g * s.O + col];
      float sum = t[0];
#pragma unroll
      for (int g = 1; g < OUT_SEGS; g++) sum += t[g];
      v.b.out[(size_t)r * s.O + col] = sum;
      sout[col] = sum;
    }
    __syncthreads();
  } else {
    const int per = (s.H + OUT_SEGS - 1) / OUT_SEGS;
    const int y0 = seg * per, y1 = min(s.H, y0 + per);
    float *out = v.b.out + (size_t)r * s.O;
    for (int c0 = 0; c0 < s.O; c0 += 64) {
      int col = c0 + lane;
      float acc0 = 0.0f, acc1 = 0.0f;
      if (col < s.O) {
        const float *w = v.b.ho_w + col;
        int y = y0;
        /* 32 rows' weights in flight per batch; the sums keep the order of the plain loop */
        for (; y + 31 < y1; y += 32) {
          float wv[32];
#pragma unroll
          for (int k = 0; k < 32; k++) wv[k] = w[(size_t)(y + k) * s.O];
#pragma unroll
          for (int k = 0; k < 32; k += 2) {
            acc0 += shid[y + k] * wv[k];
            acc1 += shid[y + k + 1] * wv[k + 1];
          }
        }
#pragma unroll 4
        for (; y + 1 < y1; y += 2) {
          acc0 += shid[y] * w[(size_t)y * s.O];
          acc1 += shid[y + 1] * w[(size_t)(y + 1) * s.O];
        }
        if (y < y1) acc0 += shid[y] * w[(size_t)y * s.O];
      }
      part[seg * 64 + lane] = acc0 + acc1;
      __syncthreads();
      if (seg == 0 && col < s.O) {
        float sum = part[lane];
        for (int g = 1; g < OUT_SEGS; g++) sum += part[g * 64 + lane];
        out[col] = sum;
        sout[col] = sum;
      }
      __syncthreads();
    }
  }
  TT_STAMP(2);
  // the backprop below needs this thread's row of W_ho: request it now (narrow output layers),
  // so that it arrives while wave 0 works out the softmax
  constexpr int TOP_PF = 12; /* float4 per row: o_size <= 48 */
  float4 wrow[TOP_PF];
  const bool top_pf = s.O <= 4 * TOP_PF;
  auto prefetch_rows = [&]() {
    if (top_pf) {
      const int y = threadIdx.x;
      const bool need = y != 0 && y < s.H && shid[y] != 0.0f;
      const float *rowp = v.b.ho_w + (size_t)(need ? y : 0) * s.O;
#pragma unroll
      for (int k = 0; k < TOP_PF; k++) wrow[k] = (need && 4 * k < s.O) ? ld4(rowp + 4 * k) : zero4();
    }
  };
  /* (tried, round 5: wave 0 asking for its rows from INSIDE the softmax, behind the exponentials, instead of 0.8 us in
   * front of it -- the softmax then starts earlier and runs slower beside the other waves' loads: 9.20 against 9.16 us
   * to its barrier) */
  prefetch_rows();
  // ---- the loss: wave 0
  if constexpr (KIND == 0) { // softmax (charmodel-predict.c:18-27, badmaths.h:71-141)
    if (seg == 0) text_softmax_wave(s, lane, shid, sout, sex, serr, v.b.o_error + (size_t)r * s.O, target, pad_oe, tstat);
    else if (seg == 1) text_count_zeros_wave(s, lane, shid, tstat);
    __syncthreads();
    if (threadIdx.x == 64) top_add_stats(v, r, tstat); /* (its loads return before the wave's backprop loads, which are issued behind them) */
  } else if constexpr (KIND == 1) { // sigmoid_rule.h: sigmoid in place on the first n outputs, slope * (target - answer)
    if (seg == 0) { /* (o_size <= 64: launcher) */
      float term = 0.0f;
      if (lane < s.O) {
        float oe = pad_oe; /* the rest of the error row stays what it was */
        if (lane < tl.n) {
          const float a = sigmoid_answer(sout[lane], FastExpDev{});
          v.b.out[(size_t)r * s.O + lane] = a;
          oe = sigmoid_error(a, mse_target);
          v.b.o_error[(size_t)r * s.O + lane] = oe;
          term = sigmoid_loss(a, mse_target);
        }
        serr[lane] = oe;
      }
      if (tl.stats) { /* (uniform over the launch) the one wave's sum */
        term = loss_wave_sum(term);
        if (lane == 0) tstat[0] = term;
      }
    }
    if (threadIdx.x == 0) trained_sh = 1;
    __syncthreads();
    if (tl.stats && threadIdx.x == 64) loss_add_stats(v, r, tstat[0]); /* (beside the backprop, as the text loss's) */
  } else if constexpr (KIND == 3) { // parrot_rule.h: tanh in place on the first n outputs, (1 - a a) (target - a)
    if (seg < 4) { /* (o_size <= 256: text_top_takes) */
      const int x = threadIdx.x;
      float term = 0.0f;
      if (x < s.O) {
        float oe = pad_oe; /* the rest of the error row stays what it was */
        if (x < tl.n) {
          const float a = dream_tanh(sout[x]);
          v.b.out[(size_t)r * s.O + x] = a;
          oe = parrot_error(a, mse_target);
          v.b.o_error[(size_t)r * s.O + x] = oe;
          term = parrot_loss(a, mse_target);
        }
        serr[x] = oe;
      }
      term = loss_wave_sum(term);
      if (lane == 0) tstat[seg] = term;
    }
    __syncthreads();
    if (threadIdx.x == 64) loss_add_stats(v, r, loss_four_waves(tstat)); /* (beside the backprop, as the text loss's) */
  } else { // k_grouped_softmax_error, operation for operation, the outputs from LDS
    if (seg == 0) {
      float *err = v.b.o_error + (size_t)r * s.O;
      if (lane < s.O) serr[lane] = pad_oe; /* (o_size <= 64: launcher) columns outside every group stay what they were */
      int wins;
      float wrong;
      const int trained = grouped_softmax_wave(lane, tl.ngroups, tl.goff, tl.gsize, tl.gt + (size_t)blockIdx.x * tl.ngroups,
                                               sout, sex, serr, FenceOneWave{}, wins, wrong);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (lane < s.O) {
        float oe = serr[lane];
        if (trained && tl.weight && lane < s.output_size) oe *= tl.weight[lane];
        serr[lane] = oe;
        err[lane] = oe;
      }
      if (lane == 0) {
        trained_sh = trained;
        if (trained) {
          v.b.stat_err[r] += wrong;
          v.b.stat_correct[r] += wins;
          v.b.stat_count[r] += trained;
          if (tl.gate && classify_gate_raises(wrong)) *tl.gate = 1u; /* (classify_train_rule.h: the reference's if (err_sum)) */
        }
      }
    }
    __syncthreads();
    /* a stream without a usable target is not trained: its rows of the error planes stay what they were, as under
     * rnn_amd_set_calc_deltas' `active` flags (k_top_backprop) */
    if (!trained_sh) return;
  }
  TT_STAMP(3);
  // ---- top-layer backprop + soft clip (recur-nn.c:199-228, 719-721)
  float sum = 0.0f;
  float ev[3] = {0.0f, 0.0f, 0.0f}; /* h_size <= 3072 per launch condition */
  for (int q = 0, y = threadIdx.x; y < s.H; y += 1024, q++) {
    float e = 0.0f;
    if (y != 0 && shid[y] != 0.0f) {
      if (top_pf && q == 0) {
#pragma unroll
        for (int k = 0; k < TOP_PF; k++) {
          if (4 * k < s.O) {
            e += wrow[k].x * serr[4 * k];
            e += wrow[k].y * serr[4 * k + 1];
            e += wrow[k].z * serr[4 * k + 2];
            e += wrow[k].w * serr[4 * k + 3];
          }
        }
      } else {
        const float *row = v.b.ho_w + (size_t)y * s.O;
        for (int x = 0; x < s.O; x += 4) {
          float4 w = ld4(row + x);
          e += w.x * serr[x];
          e += w.y * serr[x + 1];
          e += w.z * serr[x + 2];
          e += w.w * serr[x + 3];
        }
      }
      sum += fabsf(e);
    }
    ev[q] = e;
  }
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
  if (lane == 0) tred[seg] = sum;
  __syncthreads();
  TT_STAMP(4);
  float scale;
  const bool clipped = top_soft_clip(v, r, tred, scale);
  float *dst = v.b.ehi + (size_t)r * s.I; /* step 0 plane */
  for (int q = 0, y = threadIdx.x; y < s.H; y += 1024, q++)
    dst[y] = top_plane_zero(s, y) ? 0.0f : clipped ? ev[q] * scale : ev[q];
  TT_STAMP(5);
  BND_MARK(g_bnd_top, 1);
}

// ---- the text step's top launch, round 6 form (k_text_top2): W_ho once per workgroup, from registers both times --
// (its body is k_text_top2.h's: the forward + top launch, k_fwd_top.h, runs the same one)
__global__ __launch_bounds__(1024) void k_text_top2(View v, int row0, int nrows, int fwd_ks) {
  extern __shared__ float tsh[];
  const int j = blockIdx.x, r = row0 + j; /* the stream: within the call, state row */
  BND_MARK(g_bnd_top, 0);
  TT_STAMP(0);
  float4 wv[T2_NB];
  text_top2_rest<false, false>(v, j, r, nrows, fwd_ks, tsh, wv);
  BND_MARK(g_bnd_top, 1);
}

// multi_softmax_error (charmodel-multi-predict.c:17-58) after the opinion: the output row is
// n_classes heads of alphabet_len symbols.  The head of the stream's own class is always
// trained; every other head with probability `leakage`, decided by a draw from the
// stream's generator (none for the own head: the || short-circuits).  A trained head gets
// -softmax with +1 on the next symbol; the others stay zero.  The (start, len) ranges
// the reference builds for rnn_bptt_calc_deltas -- aligned, merged when they touch -- are
// left in ranges[j].  One wave per stream; every lane runs the generator redundantly so
// that the decisions are uniform.
// Eight waves per stream: wave 0 makes the leak decisions (the generator is sequential) and the
// range list while all of them clear the error row; then the trained heads are shared out over the
// waves, each head's softmax exactly as before (the sum of the exponentials in index order).
// (As one wave per stream this was 35 us for 256 streams of 50 heads, as four 15.6, as eight with a head's
// outputs loaded once and the ordered sum on float4 reads 11 us.)
constexpr int MS_WAVES = 8, MS_MAXCLS = 256; /* (eight: a stream's ~6 trained heads in one round) */
__global__ __launch_bounds__(64 * MS_WAVES) void k_multi_softmax_error(View v, int row0, int alen, int ncls,
                                                                       unsigned long long threshold,
                                                                       const int *tclass, int *ranges,
                                                                       int range_stride) {
  extern __shared__ __attribute__((aligned(16))) float exs[]; /* [MS_WAVES][alen rounded up to 4] */
  __shared__ short trained[MS_MAXCLS];
  __shared__ int ntrained;
  __shared__ float own_err_sh;
  const RamdShape &s = v.sh;
  const int j = blockIdx.x, r = row0 + j, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float *src = v.b.out + (size_t)r * s.O;
  float *err = v.b.o_error + (size_t)r * s.O;
  const int next = v.b.target[r], own = tclass[j];
  for (int i = threadIdx.x; i < s.output_size; i += 64 * MS_WAVES) err[i] = 0.0f;
  if (wave == 0) {
    /* every lane runs the generator redundantly, so that the decisions are wave-uniform */
    int *rg = ranges + (size_t)j * range_stride;
    DevRng g = reinterpret_cast<DevRng *>(v.b.rng)[r];
    int nt = 0, nr = 0, prev_start = 0, prev_len = 0;
    unsigned long long bits = 0;
    for (int c = 0; c < ncls; c++) {
      bool train = (c == own);
      if (!train) train = dev_rand64(g) < threshold;
      if (!train) continue;
      if (lane == 0) trained[nt] = (short)c;
      nt++;
      bits |= 1ull << (c & 63);
      const int offset = c * alen;
      int start = offset & ~3, end = (offset + alen + 3) & ~3;
      if (nr && prev_start + prev_len >= start) {
        prev_len = end - prev_start;
        if (lane == 0) rg[2 * (nr - 1) + 1] = prev_len;
      } else {
        prev_start = start;
        prev_len = end - start;
        if (lane == 0) {
          rg[2 * nr] = prev_start;
          rg[2 * nr + 1] = prev_len;
        }
        nr++;
      }
    }
    if (lane == 0) {
      rg[2 * nr] = -1;
      rg[2 * nr + 1] = 0;
      if (range_stride >= RAMD_HEADBITS_AT + 2 && ncls <= 64) /* (k_ho_delta_heads reads these, not the ranges) */
        head_bits_store(rg, bits);
      reinterpret_cast<DevRng *>(v.b.rng)[r] = g;
      ntrained = nt;
    }
  }
  __syncthreads(); /* the row is clear, the list is there */
  const int alenp = (alen + 3) & ~3;
  float *ex = exs + wave * alenp;
  const int nt = ntrained;
  for (int k = wave; k < nt; k += MS_WAVES) {
    const int c = trained[k], offset = c * alen;
    const float *gs = src + offset;
    if (alen <= 128) {
      /* the head's outputs once, in registers (as loads in each of the loops below they were two round trips per head) */
      const bool in0 = lane < alen, in1 = lane + 64 < alen;
      const float g0 = gs[in0 ? lane : 0], g1 = gs[in1 ? lane + 64 : 0];
      float hi = fmaxf(g0, g1), lo = fminf(g0, g1); /* (a lane without a value holds gs[0]) */
      wave_minmax(lo, hi);
      const float adj = softmax_shift(lo, hi);
      const float e0 = fast_expf_dev(g0 + adj), e1 = fast_expf_dev(g1 + adj);
      if (in0) ex[lane] = e0;
      if (in1) ex[lane + 64] = e1;
      FenceOneWave{}();
      const float sum = ordered_sum4(ex, alen, alenp); /* (as single reads in a loop the sum was the larger part of a head) */
      const float q0 = e0 / sum, q1 = e1 / sum;
      if (in0) err[offset + lane] = softmax_error(q0, lane == next);
      if (in1) err[offset + lane + 64] = softmax_error(q1, lane + 64 == next);
      if (c == own && lane == 0) own_err_sh = softmax_error(ex[next] / sum, true);
      FenceOneWave{}(); /* before this wave's next head rewrites ex */
      continue;
    }
    const float adj = softmax_shift_of(gs, alen, lane);
    for (int i = lane; i < alen; i += 64) ex[i] = fast_expf_dev(gs[i] + adj);
    FenceOneWave{}();
    const float sum = ordered_sum(ex, alen);
    for (int i = lane; i < alen; i += 64) err[offset + i] = softmax_error(ex[i] / sum, i == next);
    if (c == own && lane == 0) own_err_sh = softmax_error(ex[next] / sum, true);
    FenceOneWave{}(); /* before this wave's next head rewrites ex */
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float own_err = own_err_sh;
    float l = 1.0f - own_err;
    v.b.stat_err[r] += own_err;
    v.b.stat_ent[r] += capped_log2f_dev(l);
    v.b.stat_count[r] += 1;
  }
}

// train_channel's loss (gstclassify.c:2070-2119) for every stream: the output row is a
// few class groups; a group whose target is valid gets -softmax with +1 on the target,
// the others zeros; if any group was trained the whole error row is multiplied by the
// per-output error weights.  One wave per stream.  gt[j * ngroups + i] < 0 (or out of
// range) = "no training for this group" -- the caller decides that (target unknown,
// ignored windows, the balanced-sampling draw), as the reference's caller does.
__global__ __launch_bounds__(64) void k_grouped_softmax_error(View v, int row0, int ngroups,
                                                              const int *goff, const int *gsize,
                                                              const int *gt, const float *weight, unsigned *gate) {
  extern __shared__ float ex[]; /* [largest group] */
  const RamdShape &s = v.sh;
  const int j = blockIdx.x, r = row0 + j, lane = threadIdx.x;
  const float *src = v.b.out + (size_t)r * s.O;
  float *err = v.b.o_error + (size_t)r * s.O;
  int wins;
  float wrong;
  const int trained = grouped_softmax_wave(lane, ngroups, goff, gsize, gt + (size_t)j * ngroups, src, ex, err, FenceBlock{}, wins, wrong);
  if (trained && weight) {
    __syncthreads(); /* one wave: its own stores are ordered; this keeps the compiler honest */
    for (int q = lane; q < s.output_size; q += 64) err[q] *= weight[q];
  }
  if (lane == 0 && trained) {
    v.b.stat_err[r] += wrong;
    v.b.stat_correct[r] += wins;
    v.b.stat_count[r] += trained;
    if (gate && classify_gate_raises(wrong)) *gate = 1u; /* (classify_train_rule.h: the reference's if (err_sum)) */
  }
}

// get_cross_entropy's inner step (charmodel-predict.c:71-76): softmax of one state
// row's outputs (badmaths.h:71-111, sums in the reference's order), the probability of
// the row's target symbol, capped_log2f of it added to the row's running total.
__global__ __launch_bounds__(64) void k_xent_accumulate(View v, int r, int count_it) {
  extern __shared__ float ex[];
  const RamdShape &s = v.sh;
  const float *src = v.b.out + (size_t)r * s.O;
  int len = s.output_size;
  wave_softmax_exps(src, ex, len, threadIdx.x, FenceBlock{});
  if (threadIdx.x != 0 || !count_it) return;
  float e = ex[v.b.target[r]] / ordered_sum(ex, len);
  v.b.xent[r] += (double)capped_log2f_dev(e);
}

// rnn_char_multi_cross_entropy's inner step (charmodel-multi-predict.c:395-403): block c
// takes head c of the output row -- softmax over that head alone (badmaths.h:71-111), the
// probability of the row's target symbol, capped log2 added to acc[c].
__global__ __launch_bounds__(64) void k_multi_xent_accumulate(View v, int r, int alen, double *acc,
                                                              int count_it) {
  extern __shared__ float ex[];
  const RamdShape &s = v.sh;
  const int c = blockIdx.x;
  const float *src = v.b.out + (size_t)r * s.O + (size_t)c * alen;
  wave_softmax_exps(src, ex, alen, threadIdx.x, FenceBlock{});
  if (threadIdx.x != 0 || !count_it) return;
  float e = ex[v.b.target[r]] / ordered_sum(ex, alen);
  acc[c] += (double)capped_log2f_dev(e);
}

// rnnca's loss (gstrnnca.c:701-714, train_net; sigmoid_rule.h): fast_sigmoid_array(answer, answer, n) IN PLACE on the
// first n outputs (badmaths.h:33-44), then o_error[i] = a (1 - a) (target - a).  The public call's kernel: one thread per
// (stream, output); the rest of the error row stays as it was (zero); the statistics are left alone.
__global__ void k_sigmoid_mse_error(View v, int row0, int nrows, int n, const float *targets,
                                    int ld) {
  int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nrows * n) return;
  int j = q / n, i = q - j * n, r = row0 + j;
  float *out = v.b.out + (size_t)r * v.sh.O;
  float a = sigmoid_answer(out[i], FastExpDev{});
  out[i] = a;
  v.b.o_error[(size_t)r * v.sh.O + i] = sigmoid_error(a, targets[(size_t)j * ld + i]);
}

// A dense loss with its progress figure, a row at a time: the rule's answer IN PLACE on the first n outputs, its error into
// o_error, the row's sum of its loss terms and one count into the set's statistics (loss_add_stats).  One workgroup of four
// waves per stream, thread x taking columns x, x + 256, ... at any o_size; outputs and error columns from n on stay what
// they were.  TanhLossRule: parrot's loss (gstparrot.c:464-477, train_net: fast_tanhf, (1 - a a) (target - a)).
// SigmoidLossRule: rnnca's for rnn_amd_set_automaton_steps where the one-launch top does not take the shape --
// k_sigmoid_mse_error's arithmetic per output, so the same bits in answers and errors.
struct TanhLossRule {
  static __device__ __forceinline__ float answer(float x) { return dream_tanh(x); }
  static __device__ __forceinline__ float error(float a, float t) { return parrot_error(a, t); }
  static __device__ __forceinline__ float loss(float a, float t) { return parrot_loss(a, t); }
};
struct SigmoidLossRule {
  static __device__ __forceinline__ float answer(float x) { return sigmoid_answer(x, FastExpDev{}); }
  static __device__ __forceinline__ float error(float a, float t) { return sigmoid_error(a, t); }
  static __device__ __forceinline__ float loss(float a, float t) { return sigmoid_loss(a, t); }
};
template <class RULE>
__global__ __launch_bounds__(256) void k_dense_loss_row(View v, int row0, int nrows, int n, const float *targets, int ld) {
  __shared__ float wsum[4];
  const int j = blockIdx.x;
  if (j >= nrows) return;
  const int r = row0 + j;
  float *out = v.b.out + (size_t)r * v.sh.O;
  float *err = v.b.o_error + (size_t)r * v.sh.O;
  float term = 0.0f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float t = targets[(size_t)j * ld + i];
    const float a = RULE::answer(out[i]);
    out[i] = a;
    err[i] = RULE::error(a, t);
    term += RULE::loss(a, t);
  }
  term = loss_wave_sum(term);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = term;
  __syncthreads();
  if (threadIdx.x == 0) loss_add_stats(v, r, loss_four_waves(wsum));
}

// fill_frame's fast_sigmoid_array(answer, answer, 3) (gstrnnca.c:813-814) for state rows
__global__ void k_sigmoid_outputs(View v, int r0, int nrows, int n) {
  int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nrows * n) return;
  int j = q / n, i = q - j * n;
  float *out = v.b.out + (size_t)(r0 + j) * v.sh.O;
  out[i] = sigmoid_answer(out[i], FastExpDev{});
}

#pragma clang fp contract(fast)

extern "C" int ramd_text_top_ok(const RamdShape *sh) { return text_top_takes(sh); } /* (fwd_plan.h: the forward plan asks too) */

/* what the forward pass left in the workspace as the top kernels' fwd_ks (top_hidden_row, k_top.h): n > 0: n K slabs;
 * n < 0: one plane of sums and -n per-tile padding partials; 0: nothing, the hidden rows are complete */
static int handover_fwd_ks(RamdHandover left) { return left.partials ? -left.partials : left.planes; }

extern "C" void ramd_launch_text_top(ramd_stream_t st_, const RamdShape *sh, const RamdBuffers *b,
                                     int row0, int nrows, RamdHandover left) {
  hipStream_t st = (hipStream_t)st_;
  const int fwd_ks = handover_fwd_ks(left);
  View v = make_view(sh, b);
  /* round 6's form where its preconditions hold (k_text_top2): o_size a multiple of 4 up to 64 (sixteen lanes a row of
   * W_ho), a wave's rows of W_ho in one batch of T2_NB x 4 */
  if (text_top2_takes(sh)) { /* (fwd_top_plan.h: the forward + top launch asks the same question) */
    const size_t shm2 = (size_t)text_top2_lds_floats(sh->H, sh->O) * sizeof(float);
    RAMD_LAUNCH(k_text_top2, dim3(nrows), dim3(1024), shm2, st, v, row0, nrows, fwd_ks);
    return;
  }
  size_t shm = (size_t)(sh->H + OUT_SEGS * 64 * 4 + (OUT_SEGS + 3) * sh->O) * sizeof(float);
  RAMD_LAUNCH(k_text_top<0>, dim3(nrows), dim3(1024), shm, st, v, row0, nrows, fwd_ks, RamdTopLoss{});
}

/* the same launch with one of the other losses between the output layer and the backprop (RamdTopLoss, ramd_internal.h).
 * ramd_dense_top_ok: the launch takes the shape for this kind (and its switch is on) -- callers decide on the two-call form
 * UP FRONT with this: by the time the launch could decline (0, nothing launched), the forward pass has run for it (hidden
 * sums only) and cannot be redone.  Rnnca's loss and the class groups are one wave's work (o_size <= 64); parrot's has a
 * thread per column, so any o_size the text top takes. */
extern "C" int ramd_dense_top_ok(const RamdShape *sh, int kind) {
  return ramd_text_top_ok(sh) && (kind == RAMD_TOP_TANH_SLOPE || sh->O <= 64) && env_int("RECUR_AMD_DENSE_TOP", 1);
}

extern "C" int ramd_launch_dense_top(ramd_stream_t st_, const RamdShape *sh, const RamdBuffers *b, int row0, int nrows,
                                     RamdHandover left, const RamdTopLoss *loss) {
  if (!ramd_dense_top_ok(sh, loss->kind)) return 0;
  const int fwd_ks = handover_fwd_ks(left);
  hipStream_t st = (hipStream_t)st_;
  View v = make_view(sh, b);
  size_t shm = (size_t)(sh->H + OUT_SEGS * 64 * 4 + (OUT_SEGS + 3) * sh->O) * sizeof(float);
  RamdTopLoss tl = *loss; /* (stats and gate only for the kinds that own them) */
  if (tl.kind != RAMD_TOP_SIGMOID_MSE) tl.stats = 0;
  if (tl.kind != RAMD_TOP_CLASS_GROUPS) tl.gate = nullptr;
  if (tl.kind == RAMD_TOP_SIGMOID_MSE)
    RAMD_LAUNCH(k_text_top<RAMD_TOP_SIGMOID_MSE>, dim3(nrows), dim3(1024), shm, st, v, row0, nrows, fwd_ks, tl);
  else if (tl.kind == RAMD_TOP_CLASS_GROUPS)
    RAMD_LAUNCH(k_text_top<RAMD_TOP_CLASS_GROUPS>, dim3(nrows), dim3(1024), shm, st, v, row0, nrows, fwd_ks, tl);
  else if (tl.kind == RAMD_TOP_TANH_SLOPE)
    RAMD_LAUNCH(k_text_top<RAMD_TOP_TANH_SLOPE>, dim3(nrows), dim3(1024), shm, st, v, row0, nrows, fwd_ks, tl);
  else
    return 0;
  return 1;
}

extern "C" void ramd_launch_softmax_error(ramd_stream_t st_, const RamdShape *sh,
                                          const RamdBuffers *b, int row0, int nrows) {
  hipStream_t st = (hipStream_t)st_;
  View v = make_view(sh, b);
  RAMD_LAUNCH(k_softmax_error, dim3(nrows), dim3(64), (size_t)sh->output_size * sizeof(float), st, v,
                     row0, nrows);
}

extern "C" void ramd_launch_xent_accumulate(ramd_stream_t st_, const RamdShape *sh,
                                            const RamdBuffers *b, int row, int count_it) {
  hipStream_t st = (hipStream_t)st_;
  View v = make_view(sh, b);
  RAMD_LAUNCH(k_xent_accumulate, dim3(1), dim3(64), (size_t)sh->output_size * sizeof(float),
                     st, v, row, count_it);
}

extern "C" void ramd_launch_multi_xent_accumulate(ramd_stream_t st_, const RamdShape *sh,
                                                  const RamdBuffers *b, int row, int alphabet_len,
                                                  int n_classes, double *acc, int count_it) {
  hipStream_t st = (hipStream_t)st_;
  View v = make_view(sh, b);
  RAMD_LAUNCH(k_multi_xent_accumulate, dim3(n_classes), dim3(64), (size_t)alphabet_len * sizeof(float), st,
              v, row, alphabet_len, acc, count_it);
}

extern "C" void ramd_launch_dense_loss(ramd_stream_t st_, const RamdShape *sh, const RamdBuffers *b, int row0, int nrows,
                                       int kind, int n, const float *targets, int ld, int stats) {
  hipStream_t st = (hipStream_t)st_;
  View v = make_view(sh, b);
  if (kind == RAMD_TOP_TANH_SLOPE)
    RAMD_LAUNCH(k_dense_loss_row<TanhLossRule>, dim3(nrows), dim3(256), 0, st, v, row0, nrows, n, targets, ld);
  else if (stats)
    RAMD_LAUNCH(k_dense_loss_row<SigmoidLossRule>, dim3(nrows), dim3(256), 0, st, v, row0, nrows, n, targets, ld);
  else
    RAMD_LAUNCH(k_sigmoid_mse_error, dim3((nrows * n + 255) / 256), dim3(256), 0, st, v, row0, nrows, n, targets, ld);
}

extern "C" void ramd_launch_sigmoid_outputs(ramd_stream_t st_, const RamdShape *sh,
                                            const RamdBuffers *b, int r0, int nrows, int n) {
  hipStream_t st = (hipStream_t)st_;
  View v = make_view(sh, b);
  RAMD_LAUNCH(k_sigmoid_outputs, dim3((nrows * n + 255) / 256), dim3(256), 0, st, v, r0, nrows, n);
}

extern "C" void ramd_launch_multi_softmax_error(ramd_stream_t st_, const RamdShape *sh,
                                                const RamdBuffers *b, int row0, int nrows,
                                                int alphabet_len, int n_classes,
                                                unsigned long long threshold, const int *tclass,
                                                int *ranges, int range_stride) {
  hipStream_t st = (hipStream_t)st_;
  View v = make_view(sh, b);
  if (n_classes > MS_MAXCLS) {
    fprintf(stderr, "librecur_amd: more than %d class heads\n", MS_MAXCLS);
    abort();
  }
  RAMD_LAUNCH(k_multi_softmax_error, dim3(nrows), dim3(64 * MS_WAVES),
                     (size_t)MS_WAVES * ((alphabet_len + 3) & ~3) * sizeof(float), st, v, row0, alphabet_len, n_classes,
                     threshold, tclass, ranges, range_stride);
}

extern "C" void ramd_launch_grouped_softmax_error(ramd_stream_t st_, const RamdShape *sh,
                                                  const RamdBuffers *b, int row0, int nrows,
                                                  int ngroups, int largest, const int *goff,
                                                  const int *gsize, const int *gt,
                                                  const float *weight, unsigned *gate) {
  hipStream_t st = (hipStream_t)st_;
  View v = make_view(sh, b);
  RAMD_LAUNCH(k_grouped_softmax_error, dim3(nrows), dim3(64), (size_t)largest * sizeof(float), st,
                     v, row0, ngroups, goff, gsize, gt, weight, gate);
}
