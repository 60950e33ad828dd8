// k_text_top2.h -- the text step's top layer for one stream by one workgroup of sixteen waves, round 6 form: the device
// body that k_text_top2 (kernels_loss.hip) and the forward + top launch k_fwd_top (k_fwd_top.h) both run, so that
// the two give the same bits.  Every function here sets its own fp contract mode (off: the reference's operations one by
// one), whatever its including file has in force.
//
// k_text_top<0> by stamps (round 5): hidden row in LDS at 2.0 us, output layer 3.8, one-wave softmax 3.4, backprop 2.3, and
// with sixteen waves on a CU every phase is the vector ALU's instruction count times sixteen cycles.  Here
//   * the workgroup's rows of W_ho are requested FIRST, before the hidden row (nothing they need is computed here), 17
//     float4 per lane: wave w has rows y0 .. y0 + per - 1 of the matrix, lane (rsub, c4) of it rows y0 + rsub + 4 i and
//     columns 4 c4 .. + 3 -- sixteen lanes a row;
//   * they STAY in registers for the backprop (e[y] = sum over x of W_ho[y][x] o_error[x], recur-nn.c:199-228: the same
//     numbers, the other contraction): no second pass over W_ho, no prefetch to park across the softmax.  The sixteen
//     lanes' partial sums of sixteen rows are added by a transposing butterfly (15 exchanges instead of 64 row
//     reductions): lane c4 ends up with row y0 + rsub + 4 c4 -- a wave's 64 lanes hold 64 consecutive rows, one store;
//   * the softmax of up to 64 outputs stays in one wave's registers (text_softmax_regs: the sum of the exponentials by a
//     tree instead of in index order -- VERDICT round 5 item 3; the bar is 1e-4 element-wise, and the tests hold it);
//   * the error row is stored as it is formed; the soft clip (recur-nn.c:719-721: rare, a hot net) stores it again, scaled.
// Measured and dropped on the way (profiles/NOTES_r06.md): several streams per workgroup sharing the one copy of W_ho in its
// registers (the launch is not bound by what the L2s hand out but by vector-ALU instructions: 2 streams 16.1 us, 4 streams
// 25.7 against 11.0 with one).
// Text loss only (KIND 0), o_size <= 64, a wave's rows in one batch (h_size <= 1088): else k_text_top.
#pragma once
#include "k_common.h"
#include "k_top.h"

/* (T2_NB, text_top2_lds_floats: k_tiles.h -- the launchers' plans read them too) */
#define T2_SWZ(x, xorm) __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, x), ((xorm) << 10) | 0x1f))
__device__ __forceinline__ float dpp_row_sum16(float x) { return dpp_row_all(x, OpAdd{}); }
/* p[k]: this lane's partial sum of row k (k = 0 .. 15) of its sixteen-lane group; returns the group's sum of row c4 (the
 * lane's number in the group): a butterfly that halves the rows a lane still carries at every exchange */
__device__ __forceinline__ float transpose_sum16(const float (&p)[16], int c4) {
#pragma clang fp contract(off)
  float u[8], w[4], x[2];
  const bool b3 = c4 & 8, b2 = c4 & 4, b1 = c4 & 2, b0 = c4 & 1;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const float keep = b3 ? p[k + 8] : p[k], send = b3 ? p[k] : p[k + 8];
    u[k] = keep + T2_SWZ(send, 8);
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const float keep = b2 ? u[k + 4] : u[k], send = b2 ? u[k] : u[k + 4];
    w[k] = keep + T2_SWZ(send, 4);
  }
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const float keep = b1 ? w[k + 2] : w[k], send = b1 ? w[k] : w[k + 2];
    x[k] = keep + RAMD_DPP(send, 0x4E);
  }
  const float keep = b0 ? x[1] : x[0], send = b0 ? x[0] : x[1];
  return keep + RAMD_DPP(send, 0xB1);
}
/* text_softmax_wave (k_top.h) for o_size <= 64 without LDS round trips: lane i holds output i.  The same arithmetic value
 * by value (adjustment, fast_expf_dev, the division, +1 on the target, best guess with the lowest index on a tie); the sum
 * of the exponentials is a tree over the lanes, not the reference's index order.  Leaves the error row in serr (LDS) and
 * err (global), the statistics in tstat[0..2]. */
__device__ __forceinline__ void text_softmax_regs(const RamdShape &s, int lane, const float *sout, float *serr, float *err,
                                                  int target, float pad_oe, float *tstat) {
#pragma clang fp contract(off)
  const int len = s.output_size;
  const bool in = lane < len;
  const float o = sout[in ? lane : 0];
  const float hi = wave_all(o, OpMax{}), lo = wave_all(o, OpMin{}); /* (a lane past the outputs holds output 0) */
  const float adj = softmax_shift(lo, hi);
  const float ex = in ? fast_expf_dev(o + adj) : 0.0f;
  const float sum = wave_all(ex, OpAdd{}); /* (a tree, not the index order of ordered_sum) */
  const float e = ex / sum;
  /* the best guess: the largest e, the lowest index on a tie (badmaths.h:113-141) -- the first lane that holds the maximum */
  const float emax = wave_all(in ? e : -1.0f, OpMax{});
  const unsigned long long at = __ballot(in && e == emax);
  const int best_i = at ? __ffsll((long long)at) - 1 : 0x7fffffff;
  if (lane < s.O) {
    const float oe = in ? softmax_error(e, lane == target) : pad_oe; /* the pad of o_error stays what it was (zero) */
    if (in) err[lane] = oe;
    serr[lane] = oe;
  }
  const float et = __shfl(e, target, 64);
  if (lane == 0) text_stat_store(softmax_error(et, true), best_i == target, tstat);
}

// ---- 1. this wave's rows of W_ho: requested before anything else (nothing here waits for them)
__device__ __forceinline__ void text_top2_request(const View &v, float4 (&wv)[T2_NB]) {
  const RamdShape &s = v.sh;
  const int seg = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int rsub = lane >> 4, c4 = lane & 15, OQ = s.O >> 2;
  const bool colq = c4 < OQ;
  const int per = (s.H + 15) / 16, y0 = seg * per, y1 = min(s.H, y0 + per);
  const float *wb = v.b.ho_w + 4 * (colq ? c4 : 0);
#pragma unroll
  for (int i = 0; i < T2_NB; i++) {
    const int y = y0 + rsub + 4 * i;
    /* (a row past the wave's share is multiplied by a zero hidden value below: it has to be FINITE -- row 0 of the
     * matrix, not whatever lies behind it: a net with h_size < 16 leaves whole waves without rows, and tools/gpu_fuzz_api.py
     * seed 13616 found their out-of-range rows holding NaN) */
    wv[i] = ld4(wb + (size_t)(y < y1 ? y : 0) * s.O);
  }
}

/* wave 0 runs the softmax: the target and the pad of the error row */
struct Top2Aim {
  int target;
  float pad_oe;
};
/* (PAST_L1: the target is read past this CU's L1 -- the forward half of the SAME launch has just stored it) */
template <bool PAST_L1> __device__ __forceinline__ Top2Aim text_top2_aim(const View &v, int r) {
  const RamdShape &s = v.sh;
  const int seg = threadIdx.x >> 6, lane = threadIdx.x & 63;
  Top2Aim a = {0, 0.0f};
  if (seg == 0) {
    if constexpr (PAST_L1) a.target = __hip_atomic_load(v.b.target + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else a.target = v.b.target[r];
    a.pad_oe = v.b.o_error[(size_t)r * s.O + (lane < s.O ? lane : 0)];
  }
  return a;
}

// ---- 2 .. 5: everything behind the requests (REQUESTED: the caller has made them, text_top2_request into wv; else they
// are made here, first), for stream j of the call (state row r), by all sixteen waves.  tsh:
// text_top2_lds_floats of LDS.  PAST_L1: the hidden sums are read past this CU's L1 (another workgroup of this launch
// has just written them).  Four __syncthreads.
template <bool PAST_L1, bool REQUESTED>
__device__ __forceinline__ void text_top2_rest(const View &v, int j, int r, int nrows, int fwd_ks, float *tsh,
                                               float4 (&wv)[T2_NB]) {
#pragma clang fp contract(off)
  if constexpr (!REQUESTED) text_top2_request(v, wv);
  const Top2Aim aim = text_top2_aim<PAST_L1>(v, r);
  __shared__ float tred[16];
  __shared__ float tstat[4];
  const RamdShape &s = v.sh;
  const int seg = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int rsub = lane >> 4, c4 = lane & 15, OQ = s.O >> 2;
  const bool colq = c4 < OQ;
  float *shid = tsh;             /* [H] hidden row                        */
  float *wsum = shid + s.H;      /* [16 waves][O] the waves' column sums   */
  float *sout = wsum + 16 * s.O; /* [O] outputs, [O] output error          */
  float *serr = sout + s.O;
  const int per = (s.H + 15) / 16, y0 = seg * per, y1 = min(s.H, y0 + per);
  const int target = aim.target;
  const float pad_oe = aim.pad_oe;
  // ---- 2. the hidden row
  top_hidden_row_at<PAST_L1>(v, j, r, nrows, fwd_ks, shid, WaveSumDpp{});
  __syncthreads();
  TT_STAMP(1);
  // ---- 3. output layer (recur-nn.c:150-151): the lane's rows, then the four row groups of the wave, then the waves
  {
    float4 acc = zero4();
#pragma unroll
    for (int i = 0; i < T2_NB; i++) {
      const int y = y0 + rsub + 4 * i;
      const float hv = (colq && y < y1) ? shid[y < y1 ? y : 0] : 0.0f;
      acc.x += hv * wv[i].x;
      acc.y += hv * wv[i].y;
      acc.z += hv * wv[i].z;
      acc.w += hv * wv[i].w;
    }
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
      acc.x += __shfl_xor(acc.x, off, 64);
      acc.y += __shfl_xor(acc.y, off, 64);
      acc.z += __shfl_xor(acc.z, off, 64);
      acc.w += __shfl_xor(acc.w, off, 64);
    }
    if (rsub == 0 && colq) *reinterpret_cast<float4 *>(wsum + seg * s.O + 4 * c4) = acc;
  }
  __syncthreads();
  TT_STAMP(2);
  if (seg == 0) { /* the sixteen waves' sums in wave order, then -- the same wave -- the loss */
    if (lane < s.O) {
      float t[16];
#pragma unroll
      for (int g = 0; g < 16; g++) t[g] = wsum[g * s.O + lane];
      float sum = t[0];
#pragma unroll
      for (int g = 1; g < 16; g++) sum += t[g];
      v.b.out[(size_t)r * s.O + lane] = sum;
      sout[lane] = sum;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); /* one wave: its own LDS writes are ordered */
    // ---- 4. the loss (charmodel-predict.c:18-27, badmaths.h:71-141)
    text_softmax_regs(s, lane, sout, serr, v.b.o_error + (size_t)r * s.O, target, pad_oe, tstat);
  } else if (seg == 1) {
    text_count_zeros_wave(s, lane, shid, tstat); /* the hidden row's zeros, for the statistics */
  }
  __syncthreads();
  TT_STAMP(3);
  if (threadIdx.x == 128) top_add_stats(v, r, tstat);
  // ---- 5. top-layer backprop + soft clip (recur-nn.c:199-228, 719-721) from the rows in registers
  const float4 se = colq ? *reinterpret_cast<const float4 *>(serr + 4 * c4) : zero4();
  /* the four products of a row as two packed multiplies, said so (left to the compiler's pairing, the sixteen rows came
   * out packed in one kernel and single in the next); the sums as before: (x + y) + (z + w) */
  typedef float t2_f32x2 __attribute__((ext_vector_type(2)));
  const t2_f32x2 se_lo = {se.x, se.y}, se_hi = {se.z, se.w};
  auto row_dot = [&](const float4 &w) {
    const t2_f32x2 lo = t2_f32x2{w.x, w.y} * se_lo, hi = t2_f32x2{w.z, w.w} * se_hi;
    return (lo.x + lo.y) + (hi.x + hi.y);
  };
  float pr[16];
#pragma unroll
  for (int i = 0; i < 16; i++) pr[i] = row_dot(wv[i]);
  /* (a lane outside the columns holds zeros in se; rows past y1 are dropped below) */
  const float last = dpp_row_sum16(row_dot(wv[16]));
  const float mine = transpose_sum16(pr, c4);
  /* this lane's row: y0 + rsub + 4 c4 -- the wave's 64 lanes hold rows y0 .. y0 + 63; the seventeenth row of a group
   * (y0 + rsub + 64) is lane c4 == 0's second */
  const int ya = y0 + rsub + 4 * c4, yb = y0 + rsub + 64;
  const bool rowa = ya < y1, rowb = c4 == 0 && yb < y1;
  const float ea = (rowa && ya != 0 && shid[rowa ? ya : 0] != 0.0f) ? mine : 0.0f;
  const float eb = (rowb && yb != 0 && shid[rowb ? yb : 0] != 0.0f) ? last : 0.0f;
  float *dst = v.b.ehi + (size_t)r * s.I; /* step 0 plane */
  if (rowa) dst[ya] = top_plane_zero(s, ya) ? 0.0f : ea;
  if (rowb) dst[yb] = top_plane_zero(s, yb) ? 0.0f : eb;
  const float sum = wave_all(fabsf(ea) + fabsf(eb), OpAdd{});
  if (lane == 0) tred[seg] = sum;
  TT_STAMP(6);
  __syncthreads();
  TT_STAMP(4);
  float scale;
  if (top_soft_clip(v, r, tred, scale)) { /* rare (a hot net): the row once more, scaled */
    if (rowa) dst[ya] = top_plane_zero(s, ya) ? 0.0f : ea * scale;
    if (rowb) dst[yb] = top_plane_zero(s, yb) ? 0.0f : eb * scale;
  }
  TT_STAMP(5);
}
