// k_bptt_top.h -- stage 1 of rnn_bptt_calc_deltas: the top layer backwards.  backprop_single_layer / _sparse with the
// soft clip on the error sum (recur-nn.c:156-228, 719-721) in four forms -- k_top_backprop, k_top_backprop_ranged,
// k_top_backprop_heads and k_top_heads_partial + k_top_heads_combine, with k_top_backprop_scale behind the forms that
// share a stream's rows out -- and the top layer's weight delta (recur-nn.c:256-301): k_live_mask, k_ho_delta_heads,
// k_ho_delta_finalize.  Included by kernels_bptt.hip alone; launched by its calc_top_backprop and calc_top_delta as
// calc_plan.h picks the form.  (The fifth form, the text step's top launches, is in kernels_loss.hip and shares
// top_plane_zero and top_clip / top_clip_store, k_common.h.)
#pragma once
#include "k_common.h"

// The rules the forms share, each stated once (with head_bits, top_plane_zero, top_clip, stale_plane: k_common.h).

/* Range i of a stream's error range list as every kernel reads it: the start rounded down and the length rounded up to
 * whole float4s; a negative start ends the list (false). */
__device__ __forceinline__ bool err_range(const int *rg, int i, int &start, int &len) {
  if (rg[2 * i] < 0) return false;
  start = rg[2 * i] & ~3;
  len = (rg[2 * i + 1] + 3) & ~3;
  return true;
}

/* A hidden row's error: 0 at row 0 (the reference's loop starts at 1; step 1 of the BPTT zeroes it), the product where
 * the row's hidden value is non-zero (act), else what the sparse path leaves: the stale entry of the last BPTT run
 * (the plain path without ranges passes 0). */
__device__ __forceinline__ float top_row_value(int y, bool act, float e, float stale) {
  return (y == 0) ? 0.0f : act ? e : stale;
}

/* "The streams that trained head c, in ascending order": from each thread's `mine` (its stream of the workgroup's 256
 * trained the head) the streams' numbers within the 256 into list[], by ballot and the waves' counts; returns how many.
 * Every thread of the 256 calls it (two barriers) with its tid = 64 wave + lane; wcount: one int per wave. */
__device__ __forceinline__ int streams_of_head(bool mine, short *list, int *wcount, int tid, int wave, int lane) {
  const unsigned long long bal = __ballot(mine);
  if (lane == 0) wcount[wave] = __popcll(bal);
  __syncthreads();
  int off = 0, total = 0;
#pragma unroll
  for (int w = 0; w < 4; w++) {
    if (w < wave) off += wcount[w];
    total += wcount[w];
  }
  if (mine) list[off + __popcll(bal & ((1ull << lane) - 1ull))] = (short)tid;
  __syncthreads();
  return total;
}

// ---------------------------------------------------- K5/K6: top backprop --

// backprop_single_layer / _sparse + softclip_scale (recur-nn.c:156-228,
// 719-721).  One workgroup per stream.  Writes the (scaled) error both to
// ehi[0] (what the BPTT chain reads) and leaves err_a for the lazy write-back.
__global__ __launch_bounds__(256) void k_top_backprop(View v, int row0, const int *ranges,
                                                      int range_stride,
                                                      const unsigned char *active) {
  extern __shared__ float sh[];
  __shared__ float red[4];
  const RamdShape &s = v.sh;
  int j = blockIdx.x, r = row0 + j;
  if (active && !active[j]) return;
  if (ranges) ranges += (size_t)j * range_stride; /* 0: one list for every stream */
  float *oerr = sh;          /* [O] */
  float *herr = sh + s.O;    /* [H] */
  for (int i = threadIdx.x; i < s.O; i += 256) oerr[i] = v.b.o_error[(size_t)r * s.O + i];
  __syncthreads();
  const float *hid = v.b.hidden + (size_t)r * s.H;
  const float *old = v.b.err_a + (size_t)r * s.I;
  float sum = 0.0f;
  for (int y = threadIdx.x; y < s.H; y += 256) {
    float e; /* (top_row_value's rule as the branches around the product: this form computes it in place) */
    if (y == 0) {
      e = 0.0f;
    } else if (hid[y] != 0.0f) {
      const float *row = v.b.ho_w + (size_t)y * s.O;
      e = 0.0f;
      if (ranges) {
        /* (err_range's rule, in place: through the function this loop took 78 registers for 60) */
        for (int i = 0; ranges[2 * i] >= 0; i++) {
          int start = ranges[2 * i] & ~3, len = (ranges[2 * i + 1] + 3) & ~3;
          for (int x = 0; x < len; x++) e += row[start + x] * oerr[start + x];
          sum += fabsf(e); /* once per range, e keeps running: recur-nn.c:178-191 */
        }
      } else {
        /* a row is O contiguous floats (O % 4 == 0): whole rows as float4, same order */
        for (int x = 0; x < s.O; x += 4) {
          float4 w = ld4(row + x);
          e += w.x * oerr[x];
          e += w.y * oerr[x + 1];
          e += w.z * oerr[x + 2];
          e += w.w * oerr[x + 3];
        }
        sum += fabsf(e);
      }
    } else {
      e = ranges ? old[y] : 0.0f; /* sparse path leaves the stale value */
    }
    herr[y] = e;
  }
  sum = block_sum_256(sum, red);
  const TopClip clip = top_clip(s, sum);
  float *dst = v.b.ehi + (size_t)r * s.I; /* step 0 plane */
  for (int y = threadIdx.x; y < s.H; y += 256) dst[y] = top_plane_zero(s, y) ? 0.0f : clip.on ? herr[y] * clip.scale : herr[y];
  top_clip_store(v, r, clip);
}

// backprop_single_layer_sparse (recur-nn.c:156-196) with half a wave per hidden row: k_top_backprop
// gives every thread a row of W_ho of its own and walks the ranges' columns one by one -- 64
// lanes on 64 different cache lines per load -- which at o_size 3652 (the multi-head nets) took
// 486 us for 256 streams.  Here 32 lanes read a row's range as float4 (a head of 73 symbols is 19
// of them: one instruction per row and range), a wave works on eight rows at a time (four
// instructions, each covering two rows) so that the loads and the shuffle chains of the rows
// overlap, the products are reduced over the 32 lanes with xor shuffles (a fixed tree per range),
// and the range's sum joins the row's running value and |running value| the error sum, range by
// range as the reference does (recur-nn.c:178-191).  Rows whose hidden value is zero keep the
// stale entry of the last BPTT run.  One workgroup of 16 waves per stream; with
// few streams (a GPU's share of a sharded set, the one-net trainer) the rows of a stream are
// shared out over gridDim.y workgroups -- a row is a chain of memory round trips per range, and
// 32 busy CUs of 256 leave most of the latency exposed -- which leave the unscaled values and
// their partial sums of |e| (part) for k_top_backprop_scale.
__global__ __launch_bounds__(1024) void k_top_backprop_ranged(View v, int row0, const int *ranges,
                                                              int range_stride, const unsigned char *active,
                                                              float *part) {
  extern __shared__ __attribute__((aligned(16))) float rsh[];
  __shared__ float red[16];
  __shared__ int rlist[2 * 65];
  const RamdShape &s = v.sh;
  const int j = blockIdx.x, r = row0 + j;
  if (active && !active[j]) return;
  ranges += (size_t)j * range_stride; /* 0: one list for every stream */
  float *oerr = rsh;       /* [O] */
  float *herr = rsh + s.O; /* [H] */
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int half = lane >> 5, l32 = lane & 31;
  for (int i = threadIdx.x; i < s.O; i += 1024) oerr[i] = v.b.o_error[(size_t)r * s.O + i];
  if (threadIdx.x == 0) {
    int n = 0;
    while (n < 64 && err_range(ranges, n, rlist[2 * n], rlist[2 * n + 1])) n++;
    rlist[2 * n] = -1;
  }
  __syncthreads();
  const float *hid = v.b.hidden + (size_t)r * s.H;
  const float *old = v.b.err_a + (size_t)r * s.I;
  float sum = 0.0f; /* this half-wave's rows */
  constexpr int PAIRS = 8; /* sixteen rows at a time */
  /* this workgroup's rows: [ylo, yhi), whole groups of sixteen */
  const int nb = gridDim.y, groups = (s.H + 2 * PAIRS - 1) / (2 * PAIRS);
  const int ylo = (int)(((long)groups * blockIdx.y) / nb) * 2 * PAIRS;
  const int yhi = min(s.H, (int)(((long)groups * (blockIdx.y + 1)) / nb) * 2 * PAIRS);
  for (int y0 = ylo + 2 * PAIRS * wave; y0 < yhi; y0 += 2 * PAIRS * 16) {
    float e[PAIRS];
    bool act[PAIRS];
    const float *rowp[PAIRS];
#pragma unroll
    for (int q = 0; q < PAIRS; q++) {
      const int y = y0 + 2 * q + half; /* this half-wave's row of pair q */
      act[q] = y > 0 && y < yhi && hid[y < s.H ? y : 0] != 0.0f;
      rowp[q] = v.b.ho_w + (size_t)(act[q] ? y : 0) * s.O;
      e[q] = 0.0f;
    }
    for (int i = 0; rlist[2 * i] >= 0; i++) {
      const int start = rlist[2 * i], len4 = rlist[2 * i + 1] >> 2;
      float p[PAIRS];
#pragma unroll
      for (int q = 0; q < PAIRS; q++) p[q] = 0.0f;
      for (int x4 = l32; x4 < len4; x4 += 32) {
        const float4 o4 = ld4(oerr + start + 4 * x4);
#pragma unroll
        for (int q = 0; q < PAIRS; q++) {
          const float4 w4 = ld4(rowp[q] + start + 4 * x4);
          p[q] += (w4.x * o4.x + w4.y * o4.y) + (w4.z * o4.z + w4.w * o4.w);
        }
      }
#pragma unroll
      for (int off = 16; off > 0; off >>= 1)
#pragma unroll
        for (int q = 0; q < PAIRS; q++) p[q] += __shfl_xor(p[q], off, 64);
#pragma unroll
      for (int q = 0; q < PAIRS; q++)
        if (act[q]) {
          e[q] += p[q];
          sum += fabsf(e[q]); /* once per range, e keeps running: recur-nn.c:178-191 */
        }
    }
    if (l32 == 0) {
#pragma unroll
      for (int q = 0; q < PAIRS; q++) {
        const int y = y0 + 2 * q + half;
        /* (top_row_value's rule, in place: the stale entry is only fetched where the row is skipped) */
        if (y < yhi) herr[y] = (y == 0) ? 0.0f : act[q] ? e[q] : old[y];
      }
    }
  }
  sum += __shfl_xor(sum, 32, 64); /* the two half-waves' rows */
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  sum = ((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7]));
  sum += ((red[8] + red[9]) + (red[10] + red[11])) + ((red[12] + red[13]) + (red[14] + red[15]));
  if (nb > 1) { /* unscaled values and this workgroup's share of the sum: k_top_backprop_scale goes on */
    float *dst = v.b.ehi + (size_t)r * s.I;
    for (int y = ylo + threadIdx.x; y < yhi; y += 1024) dst[y] = top_plane_zero(s, y) ? 0.0f : herr[y];
    if (threadIdx.x == 0) part[(size_t)j * nb + blockIdx.y] = sum;
    return;
  }
  const TopClip clip = top_clip(s, sum);
  float *dst = v.b.ehi + (size_t)r * s.I; /* step 0 plane */
  for (int y = threadIdx.x; y < s.H; y += 1024) dst[y] = top_plane_zero(s, y) ? 0.0f : clip.on ? herr[y] * clip.scale : herr[y];
  top_clip_store(v, r, clip);
}

// backprop_single_layer_sparse (recur-nn.c:156-196) for a multi-head output layer as ONE fp32 MFMA GEMM over all
// streams: E_h[s][y] = sum_k o_error[s][k] W_ho[y][k] with K = the whole output row (3652 columns at 73 symbols x 50
// heads), instead of k_top_backprop_ranged's per-(stream, row, range) gathers (93 us, 480 MB of W_ho columns at
// 256 streams).  What makes that legitimate for the multi-head loss and for nothing else (launcher flag
// RAMD_RANGES_ARE_HEADS): the loss has cleared the error row outside the trained heads, so the columns between a
// stream's ranges contribute exact zeros, and its ranges -- runs of whole heads of >= 24 columns -- lie >= 16 columns
// apart.  The reference's error sum is NOT sum |e|: it adds |running value| after every range (recur-nn.c:178-191),
// so the running values at the range ends are needed, per (stream, row).  K therefore runs IN ORDER inside one
// accumulator chain per element (no split over waves or workgroups), in blocks of 16 columns, and after a block in
// which a stream's range ends -- the zeros up to the block boundary change nothing -- the lanes that hold that
// stream's rows add |accumulator| to their sums (a 32-bit mask per block says which streams: built in LDS from the
// range lists).  Workgroup = 32 streams x 32 rows: four multiplying waves with a 16 x 16 tile each
// (v_mfma_f32_16x16x4_f32) and four loader waves that stage both operands through an LDS ring in k_chain_main's
// manner, 64 columns at a time (as direct per-wave loads every wave fetched its own 16 + 16 rows: 87 us, bound by
// the traffic out of the L2); 264 workgroups at 256 streams, two per CU.  Rows whose hidden value is zero keep the stale entry of the last
// BPTT run and add nothing; the unscaled values go to error plane 0 and the per-tile sums to
// `part` for k_top_backprop_scale, as with k_top_backprop_ranged's shared-out form.
constexpr int TBH_K = 64, TBH_STAGES = 4;              /* columns per stage, stages of the ring: 64 KB, two workgroups per CU */
constexpr int TBH_STAGE_FLOATS = (32 + 32) * TBH_K;     /* 16 KB */
__global__ __launch_bounds__(512, 2) void k_top_backprop_heads(View v, int row0, int nrows, const int *ranges,
                                                               int range_stride, const unsigned char *active, float *part,
                                                               int nb, int tm) {
  __shared__ __attribute__((aligned(16))) float smem[TBH_STAGES * TBH_STAGE_FLOATS];
  extern __shared__ unsigned endmask[]; /* [KB] bit s: stream s0 + s has a range ending in this block */
  const RamdShape &s = v.sh;
  const int KB = (s.O + 15) / 16, nstages = (s.O + TBH_K - 1) / TBH_K;
  const int mt = blockIdx.x % tm, nt = blockIdx.x / tm;
  const int s0 = mt * 32, y0 = nt * 32;
  const int tid = threadIdx.x, wave8 = tid >> 6, lane = tid & 63;
  const bool loader = wave8 >= 4;
  const int wave = wave8 & 3;
  const int wr = wave >> 1, wc = wave & 1, m = lane & 15, kq = lane >> 4;
  // --- loader waves: both operands are K-contiguous rows (32 error rows, 32 rows of W_ho), staged 64 columns at a
  // time by LDS-DMA the way k_chain_main stages its operands (kernels_chain.hip): instruction i of a stage fills rows
  // 4 i .. 4 i + 3 of A (i < 8) or of B, the 16-byte chunk c of row r at position c ^ (r & 15) (conflict-free
  // ds_read_b128 of sixteen rows at once); four instructions per loader wave and stage
  const float *src[4];
  int kcol[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int i = wave * 4 + j;
    const int row = 4 * (i & 7) + (lane >> 4);
    const int c = (lane & 15) ^ (row & 15);
    const float *base = (i < 8) ? v.b.o_error + (size_t)(row0 + min(s0 + row, nrows - 1)) * s.O
                                : v.b.ho_w + (size_t)min(y0 + row, s.H - 1) * s.O;
    src[j] = base + 4 * c;
    kcol[j] = 4 * c;
  }
  auto issue = [&](int stage) {
    float *dst = smem + (stage % TBH_STAGES) * TBH_STAGE_FLOATS + wave * 4 * 256;
    const int k0 = stage * TBH_K;
#pragma unroll
    for (int j = 0; j < 4; j++) { /* chunks past the row's end come from a zero line */
      const float *g = (k0 + kcol[j] + 4 <= s.O) ? src[j] + k0 : v.b.zeros;
      __builtin_amdgcn_global_load_lds((glb_void_t *)g, (lds_void_t *)(dst + j * 256), 16, 0, 0);
    }
  };
  if (loader) {
#pragma unroll
    for (int p = 0; p < TBH_STAGES - 1; p++)
      if (p < nstages) issue(p);
  }
  for (int kb = tid; kb < KB; kb += 512) endmask[kb] = 0u;
  __syncthreads();
  if (tid < 32 && s0 + tid < nrows) {
    const int *rg = ranges + (size_t)(s0 + tid) * range_stride;
    int start, len;
    for (int i = 0; i < 64 && err_range(rg, i, start, len); i++) {
      const int end = start + len;
      int kbe = (end + 15) / 16 - 1;
      kbe = kbe < 0 ? 0 : kbe >= KB ? KB - 1 : kbe;
      atomicOr(&endmask[kbe], 1u << tid);
    }
  }
  __syncthreads();
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float sabs[4] = {0.f, 0.f, 0.f, 0.f};
  if (loader) {
    for (int st = 0; st < nstages; st++) {
      const int ahead = min(TBH_STAGES - 2, nstages - 1 - st); /* stages that may stay in flight: 4 DMAs each */
      if (ahead >= 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else if (ahead == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier(); /* stage st has landed; stage st - 1's buffer is free */
      if (st + TBH_STAGES - 1 < nstages) issue(st + TBH_STAGES - 1);
    }
    return;
  }
  const unsigned msh = 16u * (unsigned)wr + 4u * (unsigned)kq; /* this lane's four streams: bits msh .. msh + 3 */
  const uint32_t lds0 = lds_byte_addr(smem);
  const uint32_t a_off = (uint32_t)(16 * wr + m) * (TBH_K * 4u);
  const uint32_t b_off = (uint32_t)(32 * TBH_K) * 4u + (uint32_t)(16 * wc + m) * (TBH_K * 4u);
  for (int st = 0; st < nstages; st++) {
    __builtin_amdgcn_s_barrier(); /* stage st has landed */
    const uint32_t base = lds0 + (uint32_t)((st % TBH_STAGES) * TBH_STAGE_FLOATS) * 4u;
    f32x4 a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const uint32_t pos = (uint32_t)(((4 * u + kq) ^ m) * 16);
      a[u] = lds_read_b128(base + a_off + pos);
      b[u] = lds_read_b128(base + b_off + pos);
    }
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3])
                 :
                 : "memory");
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int kb = 4 * st + u;
      if (kb < KB) { /* (wave-uniform) */
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].x, b[u].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].y, b[u].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].z, b[u].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].w, b[u].w, acc, 0, 0, 0);
        const unsigned em = (endmask[kb] >> (16u * (unsigned)wr)) & 0xffffu;
        if (em) { /* a range of one of this wave's streams ends here: |running value| joins its sum */
          const unsigned mine = (endmask[kb] >> msh) & 15u;
#pragma unroll
          for (int r = 0; r < 4; r++)
            if ((mine >> r) & 1u) sabs[r] += fabsf(acc[r]);
        }
      }
    }
  }
  // accumulator register r: stream 4 kq + r of the wave's sixteen, row (column of the tile) m
  const int y = y0 + 16 * wc + m;
  float psum[4];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int sj = s0 + 16 * wr + 4 * kq + r; /* within the call's rows */
    const bool valid = sj < nrows && y < s.H && !(active && !active[sj < nrows ? sj : 0]);
    const size_t rr = (size_t)(row0 + (sj < nrows ? sj : 0));
    const float hv = v.b.hidden[rr * s.H + (y < s.H ? y : 0)];
    const bool act = valid && y > 0 && hv != 0.0f;
    if (valid) {
      const float stale = v.b.err_a[rr * s.I + y];
      v.b.ehi[rr * s.I + y] = top_plane_zero(s, y) ? 0.0f : top_row_value(y, act, acc[r], stale);
    }
    psum[r] = act ? sabs[r] : 0.0f;
  }
#pragma unroll
  for (int off = 1; off < 16; off <<= 1)
#pragma unroll
    for (int r = 0; r < 4; r++) psum[r] += __shfl_xor(psum[r], off, 64);
  if (m == 0) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int sj = s0 + 16 * wr + 4 * kq + r;
      if (sj < nrows) part[(size_t)sj * nb + 2 * nt + wc] = psum[r];
    }
  }
}

/* the end of backprop_single_layer_sparse + the soft clip (recur-nn.c:719-721) for streams whose
 * rows were shared out over nb workgroups: the partial sums in order, the scale, the row */
__global__ __launch_bounds__(256) void k_top_backprop_scale(View v, int row0, const unsigned char *active,
                                                            const float *part, int nb) {
  const RamdShape &s = v.sh;
  const int j = blockIdx.x, r = row0 + j;
  if (active && !active[j]) return;
  float sum = 0.0f;
  for (int k = 0; k < nb; k++) sum += part[(size_t)j * nb + k];
  const TopClip clip = top_clip(s, sum);
  if (clip.on) {
    float *dst = v.b.ehi + (size_t)r * s.I;
    for (int y = threadIdx.x; y < s.H; y += 256) dst[y] *= clip.scale; /* (0 stays 0) */
  }
  top_clip_store(v, r, clip);
}

// backprop_single_layer_sparse for the multi-head loss WITHOUT the zeros, in two launches.  A stream's error row is
// non-zero only in the heads it trained (its own and the few that leaked: ~6 of 50), so of k_top_backprop_heads' one
// GEMM over the whole output row (1.9 GFLOP, all of W_ho through every row tile's workgroups: 52 us at 1024 / 256 /
// 73 x 50) seven eighths are products with zeros.  Here
//   1. k_top_heads_partial: a workgroup takes head c and 128 rows of W_ho.  It lists the streams that trained the head
//      (the bit per head the loss left behind each range list, as k_ho_delta_heads does), stages W_ho[rows][head c]
//      once and the streams' error segments 32 streams at a time, and forms P[stream][c][row] = sum over the head's
//      columns on the matrix cores (wave w: rows 32 w .., v_mfma_f32_32x32x2_f32 with the streams as M).  W_ho is
//      read from memory exactly once.
//   2. k_top_heads_combine: a workgroup per stream walks its trained heads in ascending order, adds P[stream][c][.]
//      to the running values and, after a head that is not followed by the next one -- the end of one of the
//      reference's merged ranges -- adds |running value| to the row's share of the error sum (recur-nn.c:178-191);
//      then the stale entries, the sum, the soft clip (recur-nn.c:719-721) and the row, which is
//      what k_top_backprop_heads + k_top_backprop_scale left behind.
constexpr int THP_U = 10; /* (THP_ROWS: k_tiles.h) */
__global__ __launch_bounds__(256) void k_top_heads_partial(View v, int row0, int nrows, const int *ranges, int range_stride,
                                                           const unsigned char *active, int alen, int ncls, float *P) {
  extern __shared__ float thp_sh[]; /* [THP_ROWS][ld] rows of W_ho, [32][ld] error segments */
  __shared__ short list[256];
  __shared__ int wcount[4];
  const RamdShape &s = v.sh;
  const int c = blockIdx.x, y0 = blockIdx.y * THP_ROWS;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lm = lane & 31, kh = lane >> 5;
  const int col0 = c * alen, a0 = col0 & ~3, lead = col0 - a0; /* the aligned span starts `lead` columns before the head */
  const int span4 = (lead + alen + 3) >> 2;                     /* float4s of the span */
  const int ld = (4 * span4) | 1;
  float *w_sh = thp_sh, *e_sh = thp_sh + THP_ROWS * ld;
  /* the rows of W_ho: float4 t of the [THP_ROWS][span4] block (the span may reach past the head into the next one and
   * up to the padded row end: o_size is a multiple of 4).  Ten loads in flight per thread (all of the block at 73 symbols), no branch around a load
   * (see k_ho_delta_heads): what lies outside the block lands in a spare slot */
  const int dump = (THP_ROWS + 32) * ld;
  /* (the first 256 streams' head bits are asked for before the rows: one round trip less in the workgroup's chain) */
  const unsigned long long bits0 = head_bits(ranges, min(tid, nrows - 1), range_stride);
  const unsigned char live0 = active ? active[min(tid, nrows - 1)] : 1;
  for (int i0 = tid; i0 < THP_ROWS * span4; i0 += THP_U * 256) {
    float4 w[THP_U];
    int at[THP_U];
#pragma unroll
    for (int u = 0; u < THP_U; u++) {
      const int i = i0 + 256 * u;
      const bool in = i < THP_ROWS * span4;
      const int row = in ? i / span4 : 0, q = in ? i - row * span4 : 0;
      const int y = min(y0 + row, s.H - 1);
      w[u] = *reinterpret_cast<const float4 *>(v.b.ho_w + (size_t)y * s.O + a0 + 4 * q);
      at[u] = in ? row * ld + 4 * q : dump;
    }
#pragma unroll
    for (int u = 0; u < THP_U; u++) {
      float *d = w_sh + at[u];
      d[0] = w[u].x;
      d[1] = w[u].y;
      d[2] = w[u].z;
      d[3] = w[u].w;
    }
  }
  for (int base = 0; base < nrows; base += 256) {
    const int sj = base + tid, sjc = min(sj, nrows - 1);
    unsigned long long bits = bits0;
    unsigned char live = live0;
    if (base) {
      bits = head_bits(ranges, sjc, range_stride);
      live = active ? active[sjc] : 1;
    }
    const int total = streams_of_head(sj < nrows && live && ((bits >> c) & 1ull), list, wcount, tid, wave, lane);
    for (int k0 = 0; k0 < total; k0 += 32) {
      const int nk = min(32, total - k0);
      /* error segments: float4 q of stream k; what lies outside the head (the neighbours' columns) is cleared */
      {
        float4 e[5]; /* (32 streams of up to 34 float4s: 128 symbols) */
        int at[5], xs[5];
#pragma unroll
        for (int u = 0; u < 5; u++) {
          const int i = tid + 256 * u;
          const bool in = i < 32 * span4;
          const int k = in ? i / span4 : 0, q = in ? i - k * span4 : 0;
          const bool have = in && k < nk;
          e[u] = *reinterpret_cast<const float4 *>(v.b.o_error + (size_t)(row0 + base + list[k0 + (have ? k : 0)]) * s.O + a0 + 4 * q);
          at[u] = in ? k * ld + 4 * q : dump;
          xs[u] = have ? 4 * q - lead : -8; /* column of e.x within the head (-8: nothing of it) */
        }
#pragma unroll
        for (int u = 0; u < 5; u++) {
          float *d = e_sh + at[u] - (at[u] == dump ? THP_ROWS * ld : 0);
          const int x = xs[u];
          d[0] = (x >= 0 && x < alen) ? e[u].x : 0.0f;
          d[1] = (x + 1 >= 0 && x + 1 < alen) ? e[u].y : 0.0f;
          d[2] = (x + 2 >= 0 && x + 2 < alen) ? e[u].z : 0.0f;
          d[3] = (x + 3 >= 0 && x + 3 < alen) ? e[u].w : 0.0f;
        }
      }
      __syncthreads();
      f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      const float *ea = e_sh + lm * ld + kh, *wb = w_sh + (32 * wave + lm) * ld + kh;
      const int kend = 4 * span4; /* even */
#pragma unroll 4
      for (int k = 0; k < kend; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ea[k], wb[k], acc, 0, 0, 0);
      const int y = y0 + 32 * wave + lm;
      if (y < s.H) {
#pragma unroll
        for (int g = 0; g < 16; g++) {
          const int sr = (g & 3) + 8 * (g >> 2) + 4 * kh;
          if (sr < nk) P[((size_t)(row0 + base + list[k0 + sr]) * ncls + c) * s.H + y] = acc[g];
        }
      }
      __syncthreads(); /* before the next streams are staged (or the list rebuilt) */
    }
  }
}

constexpr int THC_THREADS = 320; /* a float4 of the row per thread: h_size <= 1280 in one pass (more: the loop) */
__global__ __launch_bounds__(THC_THREADS) void k_top_heads_combine(View v, int row0, const int *ranges, int range_stride,
                                                                   const unsigned char *active, int ncls, const float *P,
                                                                   int images_pending) {
  __shared__ float red[THC_THREADS / 64];
  __shared__ signed char heads[64];
  __shared__ unsigned char ends[64];
  const RamdShape &s = v.sh;
  const int j = blockIdx.x, r = row0 + j, tid = threadIdx.x;
  if (active && !active[j]) return;
  const unsigned long long bits = head_bits(ranges, j, range_stride);
  const int nh = __popcll(bits);
  if (tid < 64 && ((bits >> tid) & 1ull)) {
    const int k = __popcll(bits & ((1ull << tid) - 1ull));
    heads[k] = (signed char)tid;
    ends[k] = tid == 63 || !((bits >> (tid + 1)) & 1ull); /* not followed by the next head: one of the merged ranges ends */
  }
  __syncthreads();
  const float *Pj = P + (size_t)r * ncls * s.H;
  float *dst = v.b.ehi + (size_t)r * s.I;
  /* the stale entries: err_a as the last BPTT run left it -- which, while k_err_writeback has not rebuilt the images,
   * is one of that run's error planes (stale_plane) in columns 1 .. hidden_size, the only ones used here (plane 0 is
   * the row this thread is about to overwrite: read first).  A launch less per generation of the multi-head step. */
  const float *stale_row = v.b.err_a + (size_t)r * s.I;
  if (images_pending) {
    const int n = v.b.n_exec[r];
    if (n > 0) stale_row = v.b.ehi + ((size_t)stale_plane(n) * s.Scap + r) * s.I;
  }
  float psum = 0.0f;
  for (int y4 = 4 * tid; y4 < s.H; y4 += 4 * THC_THREADS) { /* (h_size is a multiple of 4) */
    float e[4] = {0.f, 0.f, 0.f, 0.f}, sabs[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < nh; k0 += 8) { /* eight heads' values requested together (a stream trains ~6) */
      float4 pv[8];
#pragma unroll
      for (int u = 0; u < 8; u++) pv[u] = *reinterpret_cast<const float4 *>(Pj + (size_t)heads[min(k0 + u, nh - 1)] * s.H + y4);
#pragma unroll
      for (int u = 0; u < 8; u++) {
        if (k0 + u < nh) {
          const float p[4] = {pv[u].x, pv[u].y, pv[u].z, pv[u].w};
          const bool end = ends[k0 + u];
#pragma unroll
          for (int i = 0; i < 4; i++) {
            e[i] += p[i];
            if (end) sabs[i] += fabsf(e[i]);
          }
        }
      }
    }
    const float4 hv4 = *reinterpret_cast<const float4 *>(v.b.hidden + (size_t)r * s.H + y4);
    const float4 st4 = *reinterpret_cast<const float4 *>(stale_row + y4);
    const float hv[4] = {hv4.x, hv4.y, hv4.z, hv4.w}, stale[4] = {st4.x, st4.y, st4.z, st4.w};
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int y = y4 + i;
      const bool act = y > 0 && hv[i] != 0.0f;
      o[i] = top_plane_zero(s, y) ? 0.0f : top_row_value(y, act, e[i], stale[i]);
      if (act) psum += sabs[i];
    }
    *reinterpret_cast<float4 *>(dst + y4) = make_float4(o[0], o[1], o[2], o[3]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) psum += __shfl_xor(psum, off, 64);
  if ((tid & 63) == 0) red[tid >> 6] = psum;
  __syncthreads();
  float sum = 0.0f;
#pragma unroll
  for (int w = 0; w < THC_THREADS / 64; w++) sum += red[w];
  const TopClip clip = top_clip(s, sum);
  const float scale = clip.scale;
  if (clip.on) {
    for (int y4 = 4 * tid; y4 < s.H; y4 += 4 * THC_THREADS) { /* (this thread's own entries; 0 stays 0) */
      float4 o = *reinterpret_cast<float4 *>(dst + y4);
      o.x *= scale;
      o.y *= scale;
      o.z *= scale;
      o.w *= scale;
      *reinterpret_cast<float4 *>(dst + y4) = o;
    }
  }
  top_clip_store(v, r, clip);
}

__global__ void k_live_mask(float *dst, const unsigned char *active, int n) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) dst[j] = (!active || active[j]) ? 1.0f : 0.0f;
}

// The top layer's weight deltas under the multi-head loss (recur-nn.c:256-301 with per-stream range lists): of a
// stream's error row only the heads it trained are non-zero (a handful of, say, 50), so hidden^T . o_error as a dense
// GEMM over all streams is mostly products with zero.  Here a workgroup owns head c's columns of 32 rows of ho_delta:
// it lists the streams that trained head c (the bit per head the loss left behind each range list), in ascending order
// -- the order in which the reference adds the streams' products -- stages their error segments and their 32 hidden
// values in LDS, up to 48 streams at a time with every load requested at once, and sums from there on the matrix
// cores: wave w the 32 columns 32 w .. of the head.  The untrained heads' columns get their zeros (or keep what they
// had, accumulating) from the same store.  Heads of up to 128 symbols, any number of streams.
constexpr int HDH_U = 12, HDH_K = 48; /* (20 KB of LDS at 73 symbols: seven workgroups per CU, the whole grid of 50 x 32 resident at once) */
__global__ __launch_bounds__(256) void k_ho_delta_heads(View v, int row0, int nrows, const int *ranges, int range_stride,
                                                        const unsigned char *active, int alen, int ncls, int accumulate) {
  extern __shared__ float hdh_sh[]; /* [HDH_K][alenp] error segments + 4, [HDH_K][32] hidden values + 4 */
  __shared__ short list[256];
  __shared__ int wcount[4];
  const RamdShape &s = v.sh;
  const int c = blockIdx.x, h0 = blockIdx.y * 32;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int col0 = c * alen, alenp = alen | 1; /* (an odd row stride: the staging writes spread over the banks) */
  float *e_sh = hdh_sh, *h_sh = hdh_sh + HDH_K * alenp + 4; /* (e_sh[dump], four spare floats behind h_sh) */
  const int dump = HDH_K * alenp;
  const int lm = lane & 31, kh = lane >> 5;
  const bool tile_live = 32 * wave < alen, col_live = 32 * wave + lm < alen;
  const int ecol = col_live ? 32 * wave + lm : 0;
  const int kstep = 256 / alen, xstep = 256 - kstep * alen; /* a thread's next element of an [nk][alen] block */
  f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int base = 0; base < nrows; base += 256) {
    const int sj = base + tid;
    const int sjc = min(sj, nrows - 1);
    const unsigned long long bits = head_bits(ranges, sjc, range_stride);
    const unsigned char live = active ? active[sjc] : 1;
    const int total = streams_of_head(sj < nrows && live && ((bits >> c) & 1ull), list, wcount, tid, wave, lane);
    for (int k0 = 0; k0 < total; k0 += HDH_K) {
      const int nk = min(HDH_K, total - k0);
      /* Staging without a branch: every load is made (of a clamped, valid address) and every value stored, those
       * outside the block into a spare slot behind the arrays -- under a condition the compiler sinks each load into
       * its store's branch and waits there, a round trip to the L2 per element (30 us for the kernel).
       * hidden: thread t the float4 t % 8 of streams t / 8 and 32 + t / 8; the error segments: elements
       * t + 256 u of the [nk][alen] block, HDH_U of them in flight per thread */
      float4 hq[2];
      int hat[2];
#pragma unroll
      for (int half = 0; half < 2; half++) {
        const int k = (tid >> 3) + 32 * half, q = tid & 7;
        const bool in = k < nk && h0 + 4 * q < s.H;
        const size_t rr = (size_t)(row0 + base + list[k0 + (in ? k : 0)]);
        hq[half] = *reinterpret_cast<const float4 *>(v.b.hidden + rr * s.H + (in ? h0 + 4 * q : 0));
        hat[half] = in ? k * 32 + 4 * q : HDH_K * 32;
      }
      const int n = nk * alen;
      int ek = tid / alen, ex = tid - ek * alen;
      float t[HDH_U];
      int at[HDH_U];
      auto request = [&](int i0) {
#pragma unroll
        for (int u = 0; u < HDH_U; u++) {
          const bool in = i0 + 256 * u < n;
          at[u] = in ? ek * alenp + ex : dump;
          t[u] = v.b.o_error[(size_t)(row0 + base + list[k0 + (in ? ek : 0)]) * s.O + col0 + (in ? ex : 0)];
          ek += kstep;
          ex += xstep;
          if (ex >= alen) {
            ex -= alen;
            ek++;
          }
        }
      };
      /* (the first batch by every thread, the hidden values stored with it: left behind the loop the compiler moves
       * their loads there too, one more round trip) */
      request(tid);
#pragma unroll
      for (int u = 0; u < HDH_U; u++) e_sh[at[u]] = t[u];
#pragma unroll
      for (int half = 0; half < 2; half++) *reinterpret_cast<float4 *>(h_sh + hat[half]) = hq[half];
      for (int i0 = tid + HDH_U * 256; i0 < n; i0 += HDH_U * 256) {
        request(i0);
#pragma unroll
        for (int u = 0; u < HDH_U; u++) e_sh[at[u]] = t[u];
      }
      __syncthreads();
      /* wave w: the 32 x 32 tile of columns 32 w .. of the head, two streams per v_mfma_f32_32x32x2_f32 (operand lane
       * l: stream l / 32, row or column l % 32).  As FMAs with the hidden values broadcast from LDS the sum was bound by
       * the LDS (a broadcast ds_read_b128 costs what a full one does): 10 of the kernel's 27 us. */
      if (tile_live) {
#pragma unroll 4
        for (int k = 0; k < nk; k += 2) {
          const bool in = k + kh < nk;
          const int kk = in ? k + kh : 0;
          float a = h_sh[kk * 32 + lm], bb = e_sh[kk * alenp + ecol];
          a = in ? a : 0.0f;
          bb = (in && col_live) ? bb : 0.0f;
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bb, acc, 0, 0, 0);
        }
      }
      __syncthreads(); /* before the next streams are staged (or the list rebuilt) */
    }
  }
  if (tile_live && col_live) {
#pragma unroll
    for (int g = 0; g < 16; g++) {
      const int h = h0 + (g & 3) + 8 * (g >> 2) + 4 * kh;
      if (h >= s.H) continue;
      float *d = v.b.ho_delta + (size_t)h * s.O + col0 + 32 * wave + lm;
      *d = (accumulate ? *d : 0.0f) + acc[g];
    }
  }
  /* the columns behind the last head (o_size is padded to a multiple of 4): no error ever, zero unless accumulating */
  if (c == ncls - 1 && !accumulate && tid < 32 && h0 + tid < s.H)
    for (int x = ncls * alen; x < s.O; x++) v.b.ho_delta[(size_t)(h0 + tid) * s.O + x] = 0.0f;
}

// single_layer_sgd / _sparse for all streams at once (recur-nn.c:256-301):
// hidden^T . o_error comes from the MFMA GEMM (ProbHoDelta); this sums its K
// slabs into ho_delta.  With error ranges only the columns inside a range
// receive anything.
__global__ void k_ho_delta_finalize(View v, const float *slab, int ks, int accumulate,
                                    const int *ranges) {
  const RamdShape &s = v.sh;
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  int n = s.H * s.O;
  if (e >= n) return;
  int x = e % s.O;
  float acc = accumulate ? v.b.ho_delta[e] : 0.0f;
  bool live = true;
  if (ranges) {
    live = false;
    int start, len;
    for (int i = 0; err_range(ranges, i, start, len); i++)
      if (x >= start && x < start + len) live = true;
  }
  if (live) {
    for (int z = 0; z < ks; z++) acc += slab[(size_t)z * n + e];
  }
  v.b.ho_delta[e] = acc;
}
