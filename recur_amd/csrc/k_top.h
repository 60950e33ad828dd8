// k_top.h -- the callers' softmax losses and the text model's top launch as device functions: the pieces every loss kernel
// of kernels_loss.hip and every scoring kernel of kernels_rows.hip is built from, and the phases k_text_top and k_text_top2
// share.  (Started for the fused forward + top launch that round 4 built, measured and removed: profiles/NOTES_r04.md
// section 2; callable pieces are what folding the top layer into another launch needs.)
#pragma once
#include "k_common.h"
#include "fast_exp_rule.h"
#ifndef TT_STAMP /* (development stamps of the top launches: kernels_loss.hip defines them in a PC_STAMPS build) */
#define TT_STAMP(i) do { } while (0)
#endif

// badmaths.h:14-29, kept operation for operation and ending on every float: fast_exp_rule.h.  An argument that is not
// finite gives NaN, so a softmax with an infinity or a NaN in it has NaN likelihoods and every kernel below returns.
__device__ __forceinline__ float fast_expf_dev(float x) { return fast_expf(x); }

// ---- the softmax loss in pieces (charmodel-predict.c:18-27, badmaths.h:71-141).  Every loss kernel is built from these; what
// differs between callers -- where the values lie, which reduction, which fence -- is an argument.  Each piece carries its
// own contraction mode, so that its value does not depend on the file that includes it.

/* badmaths.h:71-111: the shift that brings a row into fast_expf's domain, from the row's smallest and largest value */
__device__ __forceinline__ float softmax_shift(float lo, float hi) {
#pragma clang fp contract(off)
  if (hi > 50.0f) return 50.0f - hi;
  if (lo < -60.0f) return fminf(-60.0f - lo, 50.0f - hi);
  return 0.0f;
}
/* the lanes' (lo, hi) into the wave's, in every lane (order independent) */
__device__ __forceinline__ void wave_minmax(float &lo, float &hi) {
  for (int off = 32; off > 0; off >>= 1) {
    hi = fmaxf(hi, __shfl_xor(hi, off, 64));
    lo = fminf(lo, __shfl_xor(lo, off, 64));
  }
}
/* the shift of src[0 .. n), by one wave */
__device__ __forceinline__ float softmax_shift_of(const float *src, int n, int lane) {
  float lo = src[0], hi = src[0];
  for (int i = lane; i < n; i += 64) {
    hi = fmaxf(hi, src[i]);
    lo = fminf(lo, src[i]);
  }
  wave_minmax(lo, hi);
  return softmax_shift(lo, hi);
}
/* the exponentials of src[0 .. n) under that shift into ex (LDS), by one wave, lane-strided; then the caller's fence
 * (below) between these writes and the other lanes' reads of them */
template <class FENCE>
__device__ __forceinline__ void wave_softmax_exps(const float *src, float *ex, int n, int lane, FENCE fence) {
#pragma clang fp contract(off)
  const float adj = softmax_shift_of(src, n, lane);
  for (int i = lane; i < n; i += 64) ex[i] = fast_expf_dev(src[i] + adj);
  fence();
}
/* sum of ex[0 .. len) in index order (the reference's), the same value in every lane */
__device__ __forceinline__ float ordered_sum(const float *ex, int len) {
#pragma clang fp contract(off)
  float sum = 0.0f;
  for (int i = 0; i < len; i++) sum += ex[i];
  return sum;
}
/* the same sum on float4 reads, four in flight instead of a read per addition; ex is 16-byte aligned and readable up to
 * `cap` floats (a multiple of 4, >= len) */
__device__ __forceinline__ float ordered_sum4(const float *ex, int len, int cap) {
#pragma clang fp contract(off)
  float sum = 0.0f;
  for (int i0 = 0; 4 * i0 < len; i0 += 4) {
    float4 q[4];
#pragma unroll
    for (int i = 0; i < 4; i++) q[i] = *reinterpret_cast<const float4 *>(ex + 4 * (4 * (i0 + i) < cap ? i0 + i : 0));
#pragma unroll
    for (int i = 0; i < 4; i++) {
      if (4 * (i0 + i) + 0 < len) sum += q[i].x;
      if (4 * (i0 + i) + 1 < len) sum += q[i].y;
      if (4 * (i0 + i) + 2 < len) sum += q[i].z;
      if (4 * (i0 + i) + 3 < len) sum += q[i].w;
    }
  }
  return sum;
}
/* the error of an output with likelihood e: -softmax, +1 on the target (charmodel-predict.c:25) */
__device__ __forceinline__ float softmax_error(float e, bool is_target) {
#pragma clang fp contract(off)
  return is_target ? -e + 1.0f : -e;
}
/* capped_log2f (charmodel-helpers.h:11-13) */
__device__ __forceinline__ float capped_log2f_dev(float l) { return (l < 1e-30f) ? -100.0f : log2f(l); }
/* the best guess (badmaths.h:113-141): the largest e, the lowest index on a tie.  A lane starts from BestGuess{} and offers
 * its outputs in ascending order; wave_best_guess leaves the wave's in every lane. */
struct BestGuess {
  float e = -1.0f;
  int i = 0x7fffffff;
  __device__ __forceinline__ void offer(float oe, int oi) {
    if (oe > e) {
      e = oe;
      i = oi;
    }
  }
};
__device__ __forceinline__ void wave_best_guess(BestGuess &b) {
  for (int off = 32; off > 0; off >>= 1) {
    float oe = __shfl_xor(b.e, off, 64);
    int oi = __shfl_xor(b.i, off, 64);
    if (oe > b.e || (oe == b.e && oi < b.i)) {
      b.e = oe;
      b.i = oi;
    }
  }
}
/* fences between a wave's LDS writes and the other lanes' reads of them */
struct FenceOneWave { /* the wave is alone in its phase: its LDS operations complete in order */
  __device__ __forceinline__ void operator()() const { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
};
struct FenceBlock { /* (a one-wave workgroup: the barrier keeps the compiler honest) */
  __device__ __forceinline__ void operator()() const { __syncthreads(); }
};

// train_channel's loss (gstclassify.c:2070-2119) for one stream by ONE wave: out[] the stream's outputs (LDS or global),
// gt[ngroups] its targets; a group whose target is valid gets -softmax with +1 on the target in err[] (LDS or global), the
// others zeros.  ex[largest group] is scratch (LDS), ordered by `fence`.  Returns the number of groups trained; `wins` and
// `wrong` are their statistics.
template <class FENCE>
__device__ __forceinline__ int grouped_softmax_wave(int lane, int ngroups, const int *goff, const int *gsize, const int *gt,
                                                    const float *out, float *ex, float *err, FENCE fence, int &wins,
                                                    float &wrong) {
#pragma clang fp contract(off)
  int trained = 0;
  wins = 0;
  wrong = 0.0f;
  for (int i = 0; i < ngroups; i++) {
    const int o = goff[i], n = gsize[i], target = gt[i];
    if (target < 0 || target >= n) {
      for (int q = lane; q < n; q += 64) err[o + q] = 0.0f;
      continue;
    }
    const float *gs = out + o;
    const float adj = softmax_shift_of(gs, n, lane);
    fence(); /* (the last group's reads of ex are over) */
    for (int q = lane; q < n; q += 64) ex[q] = fast_expf_dev(gs[q] + adj);
    fence();
    const float sum = ordered_sum(ex, n);
    BestGuess best;
    for (int q = lane; q < n; q += 64) {
      float e = ex[q] / sum;
      err[o + q] = softmax_error(e, q == target);
      best.offer(e, q);
    }
    wave_best_guess(best);
    wins += (best.i == target);
    wrong += softmax_error(ex[target] / sum, true);
    trained++;
  }
  return trained;
}

// The softmax loss of one stream (charmodel-predict.c:18-27, badmaths.h:71-141) by ONE wave: sout[o_size] the
// outputs (LDS), shid[h_size] the hidden row (LDS; its zeros are counted for the statistics), target the
// stream's next symbol, pad_oe this lane's current o_error value (for the pad columns, which stay what they
// were).  Leaves the exponentials in sex, the error row in serr (LDS) and in `err` (global), and in tstat[0..3]
// the error on the target, its log2 likelihood and "best guess == target" (tstat[3], the zero count: text_count_zeros_wave).
/* the hidden row's zeros, for the statistics (tstat[3]): another wave's work beside the softmax (1.2 us of the one
 * wave's 3.4 when it counted them itself, round 5's stamps) */
__device__ __forceinline__ void text_count_zeros_wave(const RamdShape &s, int lane, const float *shid, float *tstat) {
  int zeros = 0;
  for (int i = lane; i < s.H; i += 64) zeros += (shid[i] == 0.0f);
  for (int off = 32; off > 0; off >>= 1) zeros += __shfl_down(zeros, off, 64);
  if (lane == 0) tstat[3] = (float)zeros; /* exact: h_size < 2^24 */
}
/* the statistics of a softmaxed stream for tstat[0..2]: the error on the target, its capped log2 likelihood, the hit */
__device__ __forceinline__ void text_stat_store(float target_err, bool hit, float *tstat) {
#pragma clang fp contract(off)
  const float l = 1.0f - target_err;
  tstat[0] = target_err;
  tstat[1] = capped_log2f_dev(l);
  tstat[2] = hit ? 1.0f : 0.0f;
}
__device__ __forceinline__ void text_softmax_wave(const RamdShape &s, int lane, const float *shid, const float *sout,
                                                  float *sex, float *serr, float *err, int target, float pad_oe,
                                                  float *tstat) {
#pragma clang fp contract(off)
  const int len = s.output_size;
  TT_STAMP(8);
  const float adj = softmax_shift_of(sout, len, lane);
  TT_STAMP(9);
  for (int i = lane; i < len; i += 64) sex[i] = fast_expf_dev(sout[i] + adj);
  FenceOneWave{}();
  TT_STAMP(10);
  const float sum = s.O <= 64 ? ordered_sum4(sex, len, s.O) : ordered_sum(sex, len);
  TT_STAMP(11);
  BestGuess best;
  for (int i = lane; i < s.O; i += 64) {
    float oe;
    if (i < len) {
      float e = sex[i] / sum;
      oe = softmax_error(e, i == target);
      err[i] = oe;
      best.offer(e, i);
    } else {
      oe = i < 64 ? pad_oe : err[i]; /* the pad of o_error stays what it was (zero) */
    }
    serr[i] = oe;
  }
  wave_best_guess(best);
  TT_STAMP(12);
  if (lane == 0) text_stat_store(softmax_error(sex[target] / sum, true), best.i == target, tstat);
}

// ---- the phases that both top launches (k_text_top, k_text_top2: kernels_loss.hip) run alike, one workgroup of sixteen
// waves per stream; blockIdx.x is the stream within the call, r its state row

/* a wave's sum of one value per lane, in lane 0 at least -- the two launches add k_fwd_fused's tail columns by different trees */
struct WaveSumShfl { /* six __shfl_xor steps */
  __device__ __forceinline__ float operator()(float x) const {
#pragma clang fp contract(off)
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
  }
};
struct WaveSumDpp { /* wave_sum_all: DPP within a row, then (r0 + r1) + (r2 + r3) */
  __device__ __forceinline__ float operator()(float x) const { return wave_sum_all(x); }
};
// The hidden row into shid (LDS).  fwd_ks != 0: the forward GEMM's K slabs are still in the workspace: sum them, apply the
// activation and write the hidden row here (what k_fwd_finalize does, recur-nn.c:123-148).  fwd_ks < 0: k_fwd_fused left
// one plane of sums and, for the h_size padding columns, -fwd_ks per-tile partial sums in plane 1.
/* one of the forward launch's sums.  PAST_L1: by a load that does not look in this CU's L1 -- another workgroup of the
 * SAME launch wrote the value (k_fwd_top, k_fwd_top.h); the value is the same either way */
template <bool PAST_L1> __device__ __forceinline__ float top_fwd_sum(const float *p) {
  if constexpr (PAST_L1)
    return __builtin_bit_cast(float, __hip_atomic_load(reinterpret_cast<const unsigned *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  else
    return *p;
}
/* j: the stream within the call (the row of the workspace), r: its state row */
template <bool PAST_L1, class WSUM>
__device__ __forceinline__ void top_hidden_row_at(const View &v, int j, int r, int nrows, int fwd_ks, float *shid, WSUM wave_sum) {
#pragma clang fp contract(off)
  const RamdShape &s = v.sh;
  float *hid = v.b.hidden + (size_t)r * s.H;
  if (fwd_ks != 0) {
    const float *p = v.b.slab + (size_t)j * s.H;
    const int npart = fwd_ks < 0 ? -fwd_ks : 0;
    if (fwd_ks < 0) fwd_ks = 1;
    const size_t plane = (size_t)nrows * s.H;
    for (int i = threadIdx.x; i < s.H; i += 1024) {
      /* all the slabs' loads in flight at once (a loop with a run-time trip count issues
       * them one L2 latency after another) */
      float xs[8];
#pragma unroll
      for (int z = 0; z < 8; z++) xs[z] = (z < fwd_ks) ? top_fwd_sum<PAST_L1>(p + z * plane + i) : 0.0f;
      float x = xs[0];
#pragma unroll
      for (int z = 1; z < 8; z++)
        if (z < fwd_ks) x += xs[z];
      for (int z = 8; z < fwd_ks; z++) x += top_fwd_sum<PAST_L1>(p + z * plane + i);
      if (npart && i >= s.H - 4) continue; /* the tail columns: below */
      x = act_forward(s, x);
      if (i == 0) x = 1.0f; /* the bias node, recur-nn.c:148 */
      hid[i] = x;
      shid[i] = x;
    }
    if (npart && threadIdx.x < 256) {
      /* k_fwd_fused's four tail columns (hidden value hidden_size and the padding of h_size):
       * wave p4 adds column p4's per-tile partial sums */
      const int p4 = threadIdx.x >> 6, ln = threadIdx.x & 63;
      const float *pd = v.b.slab + (size_t)nrows * s.H + (size_t)j * 4 + p4;
      float x = 0.0f;
      for (int t = ln; t < npart; t += 64) x += top_fwd_sum<PAST_L1>(pd + (size_t)t * nrows * 4);
      x = act_forward(s, wave_sum(x));
      if (ln == 0) {
        hid[s.H - 4 + p4] = x;
        shid[s.H - 4 + p4] = x;
      }
    }
  } else {
    for (int i = threadIdx.x; i < s.H; i += 1024) shid[i] = hid[i];
  }
}
/* ... by the workgroup of stream blockIdx.x of the call (the top launches) */
template <class WSUM>
__device__ __forceinline__ void top_hidden_row(const View &v, int r, int nrows, int fwd_ks, float *shid, WSUM wave_sum) {
  top_hidden_row_at<false>(v, (int)blockIdx.x, r, nrows, fwd_ks, shid, wave_sum);
}
/* the stream's running statistics of the epoch loop (charmodel-predict.c:302-304) from tstat, by one thread */
__device__ __forceinline__ void top_add_stats(const View &v, int r, const float *tstat) {
  v.b.stat_err[r] += tstat[0];
  v.b.stat_ent[r] += tstat[1];
  v.b.stat_correct[r] += (tstat[2] != 0.0f);
  v.b.stat_count[r] += 1;
  v.b.stat_zero[r] += (int)tstat[3] / (double)v.sh.hidden_size;
}
// The sixteen waves' sums of |error| (tred, behind the caller's barrier) into the stream's total -- the same tree as
// block_sum_256 within each group of four waves, then the four groups -- and the soft clip on it (top_clip).
// Thread 0 stores top_raw / top_scaled.  Returns whether the error row is clipped, and in `scale` by what.
__device__ __forceinline__ bool top_soft_clip(const View &v, int r, const float *tred, float &scale) {
#pragma clang fp contract(off)
  const float g0 = (tred[0] + tred[1]) + (tred[2] + tred[3]), g1 = (tred[4] + tred[5]) + (tred[6] + tred[7]);
  const float g2 = (tred[8] + tred[9]) + (tred[10] + tred[11]), g3 = (tred[12] + tred[13]) + (tred[14] + tred[15]);
  const TopClip clip = top_clip(v.sh, (g0 + g1) + (g2 + g3));
  top_clip_store(v, r, clip);
  scale = clip.scale;
  return clip.on;
}
