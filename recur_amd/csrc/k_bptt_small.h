// k_bptt_small.h -- stages 2 to 4 of rnn_bptt_calc_deltas (chain, extras, control, weight deltas, the error images) for
// one stream of a small net in one workgroup: bptt_and_accumulate_error, recur-nn.c:303-450.  Included by
// kernels_bptt.hip alone (behind k_extras.h: bptt_control_wave); launched by its calc_small where calc_plan.h says small.
#pragma once
#include "k_extras.h"

// ------------------------------------------ one stream, small net: one launch --
//
// bptt_and_accumulate_error (recur-nn.c:303-450) for ONE stream of a small net as one
// workgroup -- what the per-net calls of an unchanged caller need (text-predict's default net
// has 99 hidden units: D launches of a 100 x 142 matrix-vector product are all launch latency).
// The workgroup walks the steps in the reference's own order.  Thread (y = tid / 8,
// chunk = tid % 8) owns 16 columns of rows y and y + 128 of the recurrent matrix: their
// weights AND their weight-delta sums live in its registers for the whole launch, so a step
// costs it four float4 of the incoming error row and two input values from LDS, 32 + 32
// multiply-adds, and three xor shuffles per row to close the dot products (LDS bandwidth is what
// a single CU runs out of first: an earlier version that fetched the weights from LDS took
// 2.1 us per step, all of it LDS reads).  The input rows of all D steps are brought into LDS
// up front and the barriers inside the loop wait for LDS only: vmcnt counts stores too on this
// architecture, so a global load inside the loop would make every step wait for the previous
// step's plane stores.  The sum of squares closes the step and the loop ends where the
// reference's would (recur-nn.c:387-389).  The planes the other kernels read afterwards
// (error rows, extras, sums: k_err_writeback, k_bottom_error, the log) are written as the
// chain kernels write them, the control logic is the shared bptt_control_wave, and
// ih_delta (+)= ih_scale * the accumulated matrix at the end.
// Preconditions (launcher): h_size <= 128, i_size <= 256, D * i_size floats fit in LDS.
__global__ __launch_bounds__(1024) void k_bptt_small(View v, int r, int accumulate, unsigned flags,
                                                     int nx, int nxp) {
  extern __shared__ __attribute__((aligned(16))) float bsm[];
  const RamdShape &s = v.sh;
  const int I = s.I, H = s.H, hs = s.hidden_size, D = s.D;
  float *h = bsm;             /* [128] error into the step, 0 at column 0 and past hidden_size */
  float *xon = h + 128;       /* [256] the step's input row, 0 where the row is skipped or absent */
  float *en = xon + 256;      /* [256] error out of the step, by row                           */
  float *red = en + 256;      /* [16] + [1]                                                    */
  float *es_sh = red + 20;    /* [D]  sums of squares by step                                  */
  float *xall = es_sh + ((D + 3) & ~3); /* [D][I] the input rows of all the steps              */
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int y0 = tid >> 3, n0 = (tid & 7) * 16; /* rows y0, y0 + 128; columns n0 .. n0 + 15 */
  const float *W = v.b.ih_w;
  const int idx0 = v.b.idx[r];
  /* weights: rows past I and columns past H are zero */
  float w[2][16], acc[2][16];
#pragma unroll
  for (int q = 0; q < 2; q++) {
    const int y = y0 + 128 * q;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      float4 t = (y < I && n0 + 4 * k < H) ? ld4(W + (size_t)y * H + n0 + 4 * k) : zero4();
      w[q][4 * k] = t.x; w[q][4 * k + 1] = t.y; w[q][4 * k + 2] = t.z; w[q][4 * k + 3] = t.w;
    }
#pragma unroll
    for (int k = 0; k < 16; k++) acc[q][k] = 0.0f;
  }
  {
    const int I4 = I / 4;
    for (int e = tid; e < D * I4; e += 1024) {
      const int t = e / I4, i = e - t * I4;
      int slot = idx0 - t;
      if (slot < 0) slot += D;
      *reinterpret_cast<float4 *>(xall + t * I + 4 * i) = ld4(v.b.arena + ((size_t)slot * s.Scap + r) * I + 4 * i);
    }
    const float *e0 = v.b.ehi + (size_t)r * I; /* plane 0: the top layer's error */
    if (tid < 128) h[tid] = (tid == 0 || tid > hs || tid >= H) ? 0.0f : e0[tid];
    if (tid < 256) xon[tid] = 0.0f;
    for (int i = tid; i < D; i += 1024) es_sh[i] = 0.0f;
  }
  /* thresholds exactly as bptt_control_wave derives them */
  const float top = v.b.top_scaled[r];
  const float max_error_sum = MAX_ERROR_GAIN_F * top + 1;
  const float min_error_gain = MIN_ERROR_GAIN_F * top;
  const float mef_rate = v.b.mef[r] / v.b.lr[r];
  const float min_error_sum = (mef_rate < min_error_gain) ? mef_rate : min_error_gain;
  const size_t plane = (size_t)s.Scap * I;
#define LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
  const bool two_rows = (wave * 8 + 128) < I; /* this wave's second rows exist */
  __syncthreads();
  if (tid < I) { /* step 0's input row */
    const float xi = xall[tid];
    xon[tid] = act_live(s, xi) ? xi : 0.0f;
  }
  LDS_BARRIER();
  for (int t = 0; t < D; t++) {
    float sq = 0.0f;
    {
      float hv[16];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        float4 t4 = ld4(h + n0 + 4 * k);
        hv[4 * k] = t4.x; hv[4 * k + 1] = t4.y; hv[4 * k + 2] = t4.z; hv[4 * k + 3] = t4.w;
      }
#pragma unroll
      for (int q = 0; q < 2; q++) {
        if (q == 1 && !two_rows) break; /* wave-uniform */
        const float xi = xon[y0 + 128 * q];
        /* weight deltas of the step (recur-nn.c:343-358) and the error that leaves it
         * (359-376); a skipped row has xi == 0: nothing is added and its error is 0 */
        float e = 0.0f, e1 = 0.0f;
#pragma unroll
        for (int k = 0; k < 16; k += 2) {
          acc[q][k] += xi * hv[k];
          acc[q][k + 1] += xi * hv[k + 1];
          e += w[q][k] * hv[k];
          e1 += w[q][k + 1] * hv[k + 1];
        }
        e += e1;
        e = dpp_row_all<3>(e, OpAdd{}); /* the eight lanes of a row, without LDS */
        e = act_back_scale(s, xi, e);   /* (scaled before it is gated: xon holds the gated xi, zero for a skipped row) */
        e = (xi != 0.0f) ? e : 0.0f;
        if ((tid & 7) == 0) {
          en[y0 + 128 * q] = e;
          sq += e * e;
        }
      }
    }
    /* the wave's share of the sum of squares: its row leaders sit in lanes 0, 8, .., 56 */
    sq += RAMD_DPP(sq, 0x128); /* row_ror 8: lanes 0 and 8 of every row of sixteen */
    {
      const int sqi = __builtin_bit_cast(int, sq);
      float ws = __builtin_bit_cast(float, __builtin_amdgcn_readlane(sqi, 0)) +
                 __builtin_bit_cast(float, __builtin_amdgcn_readlane(sqi, 16));
      ws += __builtin_bit_cast(float, __builtin_amdgcn_readlane(sqi, 32)) +
            __builtin_bit_cast(float, __builtin_amdgcn_readlane(sqi, 48));
      if (lane == 0) red[wave] = ws;
    }
    LDS_BARRIER();
    float es = ((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7]));
    es += ((red[8] + red[9]) + (red[10] + red[11])) + ((red[12] + red[13]) + (red[14] + red[15]));
    /* the planes, laid out as the chain and extras kernels leave them; the next step's rows */
    {
      float *eo = v.b.ehi + (size_t)(t + 1) * plane + (size_t)r * I;
      if (tid >= 1 && tid <= hs) eo[tid] = en[tid];
      float *xo = v.b.ex + ((size_t)(t + 1) * s.Scap + r) * nxp;
      if (tid < nxp) xo[tid] = (tid == 0) ? en[0] : (tid < nx) ? en[hs + tid] : 0.0f;
    }
    if (tid < 128) h[tid] = (tid == 0 || tid > hs) ? 0.0f : en[tid];
    if (tid < I && t + 1 < D) {
      const float xi = xall[(t + 1) * I + tid];
      xon[tid] = act_live(s, xi) ? xi : 0.0f;
    }
    if (tid == 0) {
      es_sh[t] = es;
      v.b.esum[(size_t)t * s.Scap + r] = es;
    }
    LDS_BARRIER();
    if (es <= min_error_sum || es > max_error_sum) break; /* the same for every thread */
  }
#undef LDS_BARRIER
  if (wave == 0) {
    /* the steps that did not run left zeros, which end the scan of bptt_control_wave too */
    /* (leave_tail false: the images are written below, behind the barrier that completes the plane stores) */
    bptt_control_wave(v, r, 0, lane, bptt_control_load(v, r, 0, nullptr), flags, es_sh, 1, false);
    if (lane == 0) {
      red[16] = v.b.ih_scale[r]; /* lane 0 wrote it */
      red[17] = __int_as_float(v.b.n_exec[r]);
    }
  }
  __syncthreads(); /* (also: every plane store of this workgroup has been performed) */
  const float scale = (flags & RAMD_IH_SCALE_IN_RATE) ? 1.0f : red[16]; /* see bptt_control_wave */
  {
    /* bptt->h_error / i_error as the reference leaves them: k_err_writeback's job, from the planes
     * this workgroup has just written (nothing of them was read before: no stale lines) */
    const int nex = __float_as_int(red[17]);
    if (nex > 0 && tid < I) write_error_images(v, r, nex, nxp, tid);
  }
  float *d = v.b.ih_delta;
#pragma unroll
  for (int q = 0; q < 2; q++) {
    const int y = y0 + 128 * q;
    if (y < I) {
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if (n0 + 4 * k < H) {
          float4 *dp = reinterpret_cast<float4 *>(d + (size_t)y * H + n0 + 4 * k);
          float4 a = make_float4(acc[q][4 * k] * scale, acc[q][4 * k + 1] * scale, acc[q][4 * k + 2] * scale,
                                 acc[q][4 * k + 3] * scale);
          if (accumulate) {
            float4 o = *dp;
            a.x += o.x; a.y += o.y; a.z += o.z; a.w += o.w;
          }
          *dp = a;
        }
      }
    }
  }
}

