// k_fwd_wide.h -- the forward GEMM in 64 x 64 tiles (big sets), for the hidden layer and for a wide net's output layer.
// Included by kernels_forward.hip, which launches it (launch_fwd_wide).
//
// hidden sums = X . W_ih (recur-nn.c:117-119) for big sets of dense-input nets -- rnnca's frame
// fill is 13,824 forward-only cells of a 2048-hidden net per frame, 118 GFLOP -- on k_chain_wide's
// plan: 64 rows x 64 columns per workgroup, four multiplying waves with a 32 x 32 quadrant each
// over the whole K, four loader waves with LDS-DMA into a four-deep ring of 64-deep stages (the K loop: k_ring.h).
// A (the input rows, K-contiguous) is staged as in the chain: chunk c of row r at position
// c ^ (r & 15), one b128 read = four k.  B is W_ih itself, K-major: a stage is [64 k][64 columns]
// as it lies in memory (one DMA instruction = four k rows of 256 bytes), and a lane fetches its
// four k of a chunk with two ds_read2_b32 (as k_fwd_fused does).  K = i_size is padded to whole
// stages with zeros (chunks and rows past i_size come from a zero line); the column tiles start
// at column 0 and the last one runs past h_size, where nothing is stored.  The sums go to slab
// plane 0 for k_fwd_finalize (noise, activation, bias node).
// Preconditions (launcher): rows % 64 == 0, NS == ceil(i_size / 64).
// The same plan serves the OUTPUT layer of a wide net (the multi-head nets' 3652 columns: out = hidden . W_ho, 1.9 GFLOP
// at 256 streams, recur-nn.c:150-151): the operands come as a WideOp -- A rows K-contiguous with stride lda, B K-major
// with stride ldb, K and N their extents, C with stride ldc -- and the full K in every workgroup means the tile is the
// result (no K slabs to add up).  a == nullptr: the hidden layer's operands, from the View.
#pragma once
#include "k_ring.h"

struct WideOp {
  const float *a; /* [rows][lda], K contiguous */
  const float *b; /* [K][ldb]                  */
  float *c;       /* [rows][ldc]               */
  int lda, ldb, ldc, K, N;
};
template <int NS>
__global__ __launch_bounds__(512) void k_fwd_wide(const View *__restrict__ vp, int uniform_idx, int row0, int nrows, int tm, int tn, WideOp op) {
  extern __shared__ __attribute__((aligned(16))) float wsm[];
  View v = *vp;
  v.b.uniform_idx = uniform_idx;
  const RamdShape &s = v.sh;
  const bool hidden_layer = op.a == nullptr;
  const int opK = hidden_layer ? s.I : op.K, opN = hidden_layer ? s.H : op.N;
  const int ldb = hidden_layer ? s.H : op.ldb, ldc = hidden_layer ? s.H : op.ldc;
  const float *opB = hidden_layer ? v.b.ih_w : op.b;
  float *opC = hidden_layer ? v.b.slab : op.c;
  /* Blocks are dealt round-robin over the 8 XCDs and an XCD runs 32 workgroups at a time: those 32
   * are a supertile of 4 row tiles x 8 column tiles, so that while they walk K together every
   * stage of the input rows is fetched into that XCD's L2 once per 8 workgroups and every stage of
   * W once per 4 (one column tile after another for all the row tiles, as the chain's mapping
   * does, re-reads the whole input set once per column tile: 3.8 GB for a 13,824-cell frame). */
  const int L = blockIdx.x;
  const int xcd = L & 7, q = L >> 3;
  const int st_i = (q >> 5) * 8 + xcd, in_i = q & 31;
  const int stm = (tm + 3) >> 2;
  const int mt = (st_i % stm) * 4 + (in_i & 3), nt = (st_i / stm) * 8 + (in_i >> 2);
  if (mt >= tm || nt >= tn) return;
  const int m0 = mt * WM, n0 = nt * WN;
  const int wave8 = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool loader = wave8 >= 4;
  const int wave = wave8 & 3;
  const int lm = lane & 31, kh = lane >> 5;
  const uint32_t lds0 = lds_byte_addr(wsm);

  if (loader) {
    // instruction i (0..31): i < 16: rows 4 i .. + 3 of A (lane l: chunk (l & 15) ^ (row & 15) of
    // row 4 i + (l >> 4)); i >= 16: k rows 4 (i - 16) .. + 3 of B (lane l: 16-byte piece l & 15 of
    // k row 4 (i - 16) + (l >> 4), i.e. columns n0 + 4 (l & 15) ..)
    const float *src[8];
    int kofs[8]; /* A: first k of this lane's chunk within a stage; B: this lane's k row within a stage */
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int i = wave * 8 + j;
      if (i < 16) {
        const int row = 4 * i + (lane >> 4);
        const int c = (lane & 15) ^ (row & 15);
        src[j] = (hidden_layer ? input_row<false>(v, row0 + m0 + row, 0) : op.a + (size_t)(m0 + row) * op.lda) + 4 * c;
        kofs[j] = 4 * c;
      } else {
        const int k = 4 * (i - 16) + (lane >> 4);
        src[j] = opB + (size_t)k * ldb + n0 + 4 * (lane & 15);
        kofs[j] = k;
      }
    }
    auto issue = [&](int stage) {
      float *dst = wsm + (stage % W_STAGES) * W_STAGE_FLOATS + wave * 8 * 256;
      const int k0 = stage * WK;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const bool a_side = wave * 8 + j < 16;
        const float *g = a_side ? src[j] + k0 : src[j] + (size_t)k0 * ldb;
        if ((k0 + WK > opK && k0 + kofs[j] >= opK) || (!a_side && n0 + 4 * (lane & 15) >= opN))
          g = v.b.zeros + 4 * (lane & 15); /* past K, or past the last column of W: zeros */
        __builtin_amdgcn_global_load_lds((glb_void_t *)g, (lds_void_t *)(dst + j * 256), 16, 0, 0);
      }
    };
#pragma unroll
    for (int p = 0; p < W_STAGES - 1; p++)
      if (p < NS) issue(p);
    RING_LOADER_LOOP(W_STAGES, NS, issue)
    __syncthreads();
    return;
  }

  // ------------------------------------------------------------------ multiply
  const int wm = wave >> 1, wn = wave & 1;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; i++) acc[i] = 0.0f;
  const uint32_t arow = (uint32_t)(wm * 32 + lm) * (WK * 4u);
  const uint32_t bcol = (uint32_t)(WM * WK + wn * 32 + lm) * 4u; /* B: [k][64 columns] behind A */
  struct Frag { f32x4 a[8]; f32x2 b0[8], b1[8]; };
  auto rd = [&](int st, Frag &f) {
    const uint32_t base = lds0 + (uint32_t)((st % W_STAGES) * W_STAGE_FLOATS) * 4u;
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int c = 2 * u + kh; /* chunk = k 4 c .. 4 c + 3 of the stage, on both operands */
      f.a[u] = lds_read_b128(base + arow + (uint32_t)((c ^ (lm & 15)) * 16));
      const uint32_t baddr = base + bcol + (uint32_t)(4 * c) * (WN * 4u);
      f.b0[u] = lds_read2_b32_w64(baddr);     /* k, k + 1 */
      f.b1[u] = lds_read2_b32_w64_hi(baddr);  /* k + 2, k + 3 */
    }
  };
  auto step = [&](int st, Frag &f, Frag &fn) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); /* this stage's fragments have arrived */
    if (st + 1 < NS) {
      __builtin_amdgcn_s_barrier(); /* stage st + 1 has landed */
      rd(st + 1, fn);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 8; u++) mfma_k4(acc, f.a[u], f.b0[u].x, f.b0[u].y, f.b1[u].x, f.b1[u].y);
    __builtin_amdgcn_sched_barrier(0);
  };
  RING_READ_AHEAD(NS, Frag, rd, step)
  // the tile through LDS (the ring buffer stage NS would have used was read four barriers ago)
  float *red = wsm + (NS % W_STAGES) * W_STAGE_FLOATS; /* [64][64] */
#pragma unroll
  for (int g = 0; g < 16; g++) {
    const int row = wm * 32 + (g & 3) + 8 * (g >> 2) + 4 * kh;
    red[row * WN + wn * 32 + lm] = acc[g];
  }
  __syncthreads();
  const int etid = threadIdx.x, rq = etid >> 4, c4 = (etid & 15) * 4;
  if (n0 + c4 < opN) { /* h_size % 4 == 0, o_size % 4 == 0: whole float4s */
#pragma unroll
    for (int rr = 0; rr < 4; rr++) {
      const int row = 4 * rq + rr;
      *reinterpret_cast<float4 *>(opC + (size_t)(m0 + row) * ldc + n0 + c4) = ld4(red + row * WN + c4);
    }
  }
}
