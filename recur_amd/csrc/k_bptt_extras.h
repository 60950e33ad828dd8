// k_bptt_extras.h -- stage 3 of rnn_bptt_calc_deltas, where the one-launch chain did not take it into its tail: the
// chain "extras" (column 0 and the input columns of every step's error, recur-nn.c:338-376) and the data-dependent
// control of bptt_and_accumulate_error (recur-nn.c:317-330, 383-413) as kernels on top of k_extras.h's device
// functions.  Included by kernels_bptt.hip alone; launched by its calc_extras_control as calc_plan.h picks the form
// (k_extras_control; k_extras_dense or the generic GEMM + k_extras_finalize, then k_bptt_control).
#pragma once
#include "k_extras.h"

// Finalize of the extras GEMM: applies the row rule to column 0 and the input
// columns, keeps the raw values in ex[t+1][s][c] (for the h_error / i_error
// images) and adds their squares as the last partial sum.  One wave per (t, s).
__global__ __launch_bounds__(64) void k_extras_finalize(View v, int row0, int nrows, int nx, int nxp,
                                                        int ks, int tn) {
  const RamdShape &s = v.sh;
  int m = blockIdx.x;
  int t = m / nrows, j = m - t * nrows, r = row0 + j;
  int M = s.D * nrows;
  const float *x = input_row<false>(v, r, t);
  float *dst = v.b.ex + ((size_t)(t + 1) * s.Scap + r) * nxp;
  float sq = 0.0f;
  for (int c = threadIdx.x; c < nx; c += 64) {
    float e = 0.0f;
    for (int z = 0; z < ks; z++) e += v.b.slab[((size_t)z * M + m) * nxp + c];
    int n = c == 0 ? 0 : s.hidden_size + c;
    e = act_backward(s, x[n], e);
    dst[c] = e;
    sq += e * e;
  }
  for (int off = 32; off > 0; off >>= 1) sq += __shfl_down(sq, off, 64);
  /* the step's total: the column-tile partials of k_chain_main in index order, then
   * the extras (a fixed order, so the break decisions are reproducible); tn == 0: the one-launch
   * chain left no partials, the hidden columns' part is summed from the row */
  const float hsq = tn == 0 ? row_sumsq_load(v, t + 1, r, threadIdx.x) : 0.0f;
  if (threadIdx.x == 0) {
    float sum = hsq;
    for (int p = 0; p < tn; p++) sum += v.b.esum_part[((size_t)t * (tn + 1) + p) * s.Scap + r];
    v.b.esum[(size_t)t * s.Scap + r] = sum + sq;
  }
}

// The extras of nets with DENSE inputs (audio features, pixels: every input row counts, so the gather form has
// nothing to skip) as one launch: the GEMM [D x streams rows of the error planes] x [W_ih's bias row and input rows]^T
// with K = h_size, N = 1 + the inputs (33 for gstclassify, 36 for rnnca), and k_extras_finalize's work on its result.
// As k_gemm<ProbExtras> (64 x 64 tiles: one column tile, nine tenths of it padding, a K split and its slabs) + the
// finalize launch this was 47 + 13 us at 2048 / 512 / 10 and 13 + 6 us at 512 / 128 / 30.
// Workgroup = 16 or 32 (step, stream) rows x up to 48 columns, eight waves that each take every eighth 16-deep K chunk
// (v_mfma_f32_16x16x4_f32: 1 or 2 row tiles x 3 column tiles per wave), operands straight from memory as float4s -- a lane's
// four k of a chunk go to the chunk's four MFMAs, the same permutation of k on both sides -- four chunks in flight;
// the waves' sums meet in LDS, then 8 threads per row apply the row rule, store ex, and add the squares to the
// row's total (with the chain's partial sums, or the row's own sum of squares where it left none).
constexpr int XD_PF = 8, XD_WAVES = 8; /* (XD_NT: k_tiles.h) */
/* (round 5: eight chunks in flight instead of four, and nothing in the epilogue waits for memory on its own -- the input
 * values of the row rule are requested before the K loop, the step's total apart from the extras (the chain's partial sums,
 * or the output row's sum of squares) is formed by ALL threads behind the loop, 32 or 16 per row, every load of a thread in
 * flight at once: as eight threads per row with two loads per trip that sum was 8 dependent round trips, half of the
 * launch's 11 us at 512 / 128 / 30; 27 -> ... us at 2048 / 512 / 10) */
template <int XD_MT> /* row tiles of 16 per workgroup: 2 where that still makes 128 workgroups (W_ih's rows are fetched by half as many), else 1 */
__global__ __launch_bounds__(64 * XD_WAVES) void k_extras_dense(View v, int row0, int nrows, int nx, int nxp, int tn, int t0, int nt) {
  constexpr int XD_ROWS = 16 * XD_MT;
  constexpr int TPR = 64 * XD_WAVES / XD_ROWS; /* threads per row for the step's total */
  __shared__ float red[XD_WAVES][XD_ROWS][16 * XD_NT + 1];
  __shared__ float oth_sh[XD_ROWS];
  const RamdShape &s = v.sh;
  /* rows: steps t0 .. t0 + nt - 1 of the call's streams (one launch for all steps, or one per step beside the chain) */
  const int M = nt * nrows;
  const int m0 = blockIdx.x * XD_ROWS;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lm = lane & 15, kq = lane >> 4;
  // operand rows of this lane: two error rows, three rows of W_ih
  const float *arow[XD_MT], *brow[XD_NT];
#pragma unroll
  for (int i = 0; i < XD_MT; i++) {
    const int m = min(m0 + 16 * i + lm, M - 1);
    const int t = t0 + m / nrows, j = m % nrows;
    arow[i] = v.b.ehi + ((size_t)t * s.Scap + row0 + j) * s.I;
  }
#pragma unroll
  for (int jn = 0; jn < XD_NT; jn++) {
    const int c = 16 * jn + lm;
    brow[jn] = v.b.ih_w + (size_t)((c == 0 || c >= nx) ? 0 : s.hidden_size + c) * s.H; /* (columns >= nx: discarded below) */
  }
  f32x4 acc[XD_MT][XD_NT];
#pragma unroll
  for (int i = 0; i < XD_MT; i++)
#pragma unroll
    for (int jn = 0; jn < XD_NT; jn++) acc[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nchunks = (s.H + 15) / 16; /* h_size is a multiple of 4: a lane's float4 is inside the row or wholly past it */
  const int mine = (nchunks - wave + XD_WAVES - 1) / XD_WAVES; /* chunks wave, wave + XD_WAVES, .. */
  float4 fa[XD_PF][XD_MT], fb[XD_PF][XD_NT];
  auto request = [&](int slot, int n) {
    const int k = 16 * (wave + XD_WAVES * n) + 4 * kq;
    const bool in = n < mine && k < s.H;
    const int kc = in ? k : 0;
#pragma unroll
    for (int i = 0; i < XD_MT; i++) fa[slot][i] = ld4(in ? arow[i] + k : v.b.zeros); /* (a select on the address: one on the value would wait for it here) */
#pragma unroll
    for (int jn = 0; jn < XD_NT; jn++) fb[slot][jn] = ld4(brow[jn] + kc);
  };
#pragma unroll
  for (int p = 0; p < XD_PF; p++) request(p, p);
  // the epilogue's row (eight threads per row: columns sub, sub + 8, ..) and the input values its rule asks for
  const int row = (tid >> 3) & (XD_ROWS - 1), sub = tid & 7;
  const int m = m0 + row;
  const bool live = m < M;
  const int mm = live ? m : M - 1;
  const int t = t0 + mm / nrows, j = mm % nrows, r = row0 + j;
  constexpr int XD_CPT = (16 * XD_NT + 7) / 8; /* columns per thread */
  float xv[XD_CPT];
  if (tid < 8 * XD_ROWS) {
    const float *x = input_row_auto(v, r, t);
#pragma unroll
    for (int q = 0; q < XD_CPT; q++) {
      const int c = sub + 8 * q;
      xv[q] = x[(c == 0 || c >= nx) ? 0 : s.hidden_size + c];
    }
  }
  for (int n0 = 0; n0 < mine; n0 += XD_PF) {
#pragma unroll
    for (int p = 0; p < XD_PF; p++) {
      if (n0 + p < mine) { /* (wave-uniform) */
        float4 a[XD_MT], bb[XD_NT];
#pragma unroll
        for (int i = 0; i < XD_MT; i++) a[i] = fa[p][i];
#pragma unroll
        for (int jn = 0; jn < XD_NT; jn++) bb[jn] = fb[p][jn];
        request(p, n0 + p + XD_PF);
#pragma unroll
        for (int i = 0; i < XD_MT; i++)
#pragma unroll
          for (int jn = 0; jn < XD_NT; jn++) {
            acc[i][jn] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].x, bb[jn].x, acc[i][jn], 0, 0, 0);
            acc[i][jn] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].y, bb[jn].y, acc[i][jn], 0, 0, 0);
            acc[i][jn] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].z, bb[jn].z, acc[i][jn], 0, 0, 0);
            acc[i][jn] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].w, bb[jn].w, acc[i][jn], 0, 0, 0);
          }
      }
    }
  }
  // accumulator register r of tile (i, jn): row 16 i + 4 kq + r, column 16 jn + lm
#pragma unroll
  for (int i = 0; i < XD_MT; i++)
#pragma unroll
    for (int jn = 0; jn < XD_NT; jn++)
#pragma unroll
      for (int rr = 0; rr < 4; rr++) red[wave][16 * i + 4 * kq + rr][16 * jn + lm] = acc[i][jn][rr];
  /* the step's total apart from the extras: the chain's column-tile partials, or (tn == 0: the one-launch chain leaves
   * none) the sum of squares of the step's OUTPUT row, error plane t + 1 -- TPR threads per row, a fixed tree */
  {
    const int orow = tid / TPR, osub = tid % TPR;
    const int om = min(m0 + orow, M - 1);
    const int ot = t0 + om / nrows, orr = row0 + om % nrows;
    float o = 0.0f;
    if (tn == 0) {
      const float *erow = v.b.ehi + ((size_t)(ot + 1) * s.Scap + orr) * s.I;
      const int n4 = s.H / 4;
      constexpr int NB = 9; /* float4 per thread and batch: h_size <= 1152 in one batch of 32 threads */
      for (int b0 = osub; b0 < n4; b0 += TPR * NB) {
        float4 e[NB];
#pragma unroll
        for (int i = 0; i < NB; i++) {
          const int k4 = b0 + i * TPR;
          e[i] = ld4(k4 < n4 ? erow + 4 * k4 : v.b.zeros);
        }
#pragma unroll
        for (int i = 0; i < NB; i++) o += (e[i].x * e[i].x + e[i].y * e[i].y) + (e[i].z * e[i].z + e[i].w * e[i].w);
      }
    } else {
      float pv[3]; /* (tn <= 33 column tiles, TPR >= 16) */
#pragma unroll
      for (int i = 0; i < 3; i++) {
        const int p = osub + i * TPR;
        pv[i] = p < tn ? v.b.esum_part[((size_t)ot * (tn + 1) + p) * s.Scap + orr] : 0.0f;
      }
      o = (pv[0] + pv[1]) + pv[2];
      for (int p = osub + 3 * TPR; p < tn; p += TPR) o += v.b.esum_part[((size_t)ot * (tn + 1) + p) * s.Scap + orr];
    }
#pragma unroll
    for (int off = 1; off < TPR; off <<= 1) o += __shfl_xor(o, off, 64);
    if (osub == 0) oth_sh[orow] = o;
  }
  __syncthreads();
  if (tid >= 8 * XD_ROWS) return;
  float *dst = v.b.ex + ((size_t)(t + 1) * s.Scap + r) * nxp;
  float sq = 0.0f;
#pragma unroll
  for (int q = 0; q < XD_CPT; q++) {
    const int c = sub + 8 * q;
    if (c < nx) {
      float e = 0.0f;
#pragma unroll
      for (int w = 0; w < XD_WAVES; w++) e += red[w][row][c];
      e = act_backward(s, xv[q], e);
      if (live) dst[c] = e;
      sq += e * e;
    }
  }
#pragma unroll
  for (int off = 1; off < 8; off <<= 1) sq += __shfl_xor(sq, off, 64);
  if (sub == 0 && live) v.b.esum[(size_t)t * s.Scap + r] = oth_sh[row] + sq;
}

/* (t0, nt: steps t0 .. t0 + nt - 1.  One launch per step on a second stream beside a launch-per-step chain was tried --
 * hidden 2048: 10 steps of 40 us -- and lost: the chain's workgroups fill every CU's LDS, the extras' wait for a step to
 * end and delay the next: 890 -> 1004 us per generation at 2048 / 512 / 10.  profiles/NOTES_r05.md) */
static void ramd_launch_extras_dense(hipStream_t st, const View &v, const RamdShape *sh, int row0, int nrows, int nx, int nxp,
                                     int tn_parts, int t0, int nt) {
  const int M = nt * nrows;
  if (M / 32 >= 128)
    RAMD_LAUNCH(k_extras_dense<2>, dim3((M + 31) / 32), dim3(64 * XD_WAVES), 0, st, v, row0, nrows, nx, nxp, tn_parts, t0, nt);
  else
    RAMD_LAUNCH(k_extras_dense<1>, dim3((M + 15) / 16), dim3(64 * XD_WAVES), 0, st, v, row0, nrows, nx, nxp, tn_parts, t0, nt);
}

__global__ __launch_bounds__(256) void k_bptt_control(View v, int row0, int nrows,
                                                      const unsigned char *active, unsigned flags,
                                                      int tn) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= nrows) return;
  const int r = row0 + j;
  bptt_control_wave(v, r, j, lane, bptt_control_load(v, r, j, active), flags, v.b.esum + r, (size_t)v.sh.Scap);
}

// The extras' gather and k_bptt_control in one launch, one workgroup per stream: the waves
// share out the stream's steps, leave each step's error sum in LDS, and wave 0 then runs
// the control logic on them (nothing else needs the sums of other streams).  The body is
// extras_control_stream (k_extras.h), which the one-launch chain also runs in its tail.
template <int MAXQ, int THREADS>
__global__ __launch_bounds__(THREADS) void k_extras_control(View v, int row0, int nrows, int nx,
                                                            int nxp, int tn,
                                                            const unsigned char *active,
                                                            unsigned flags) {
  extern __shared__ float es_sh[]; /* [D] the steps' totals; tn == 0: then [D + 1] the rows' own sums of squares */
  const int j = blockIdx.x;
  extras_control_stream<MAXQ, THREADS>(v, row0 + j, j, nx, nxp, tn, active, flags, es_sh);
}

