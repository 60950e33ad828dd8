// k_chain_steps.h -- the BPTT chain a launch per step: k_chain_main (32 x 32 tiles) and k_chain_wide (64 x 64 tiles, big
// sets), included by kernels_chain.hip, which launches them.  Their K loop is k_ring.h's.
#include "k_ring.h"
// ------------------------------------------------------ BPTT chain step --
//
// One launch per BPTT step t (recur-nn.c:338-376 for every stream at once):
//     E[t+1][s][y] = on(X_t[s][y]) * sum_k E[t][s][k] W_ih[y][k],   y = 1..hidden_size
// plus the per-stream sum of squares.  The hidden->hidden block is all the next
// step needs, and for a power-of-two hidden size it tiles exactly: 32 x 32
// output tiles, (S/32) x (hidden/32) workgroups = 256 at the 1024 / 256 size,
// one per CU, no split-K slabs and no separate finalize pass.  Column 0 (bias
// row) and the real-input rows only feed the sum of squares and are done for
// all steps together afterwards (k_extras_control, or the ProbExtras GEMM for very wide nets).
//
// Workgroup = 8 waves.  Waves 0-3 multiply: each takes a quarter of every 128-deep K
// stage (in-workgroup split-K, summed through LDS at the end).  Waves 4-7 only move data:
// operand stages go global -> LDS by LDS-DMA (global_load_lds_dwordx4, no VGPR round
// trip), three stages deep, with counted s_waitcnt vmcnt and raw s_barrier so that two
// stages stay in flight across barriers.  LDS rows are 128 floats; the 16-byte chunk c
// of row r is stored at chunk position c ^ (r & 15), applied on the DMA's global
// address (the LDS side of a DMA is lane-linear) and again on the ds_read_b128
// address, which makes the 16-lane groups of ds_read_b128 conflict free.
// Fragments are fetched with inline-asm ds_read_b128 one stage ahead of the MFMAs that
// use them (hipcc would otherwise drain vmcnt to 0 before any LDS read that may alias an
// LDS-DMA destination, and would not overlap the reads with the previous stage's MFMAs).

// The View is read from device memory instead of coming by value: 520 bytes of kernel
// arguments per launch are fetched from the host-visible argument ring, and this kernel is
// launched D times per generation.  Only the ring position changes between generations, and
// that comes as a plain argument.
template <bool UNI, int NS = 0> /* NS > 0: the number of K stages, known at compile time */
__global__ __launch_bounds__(512) void k_chain_main(const View *__restrict__ vp, int uniform_idx,
                                                    int row0, int nrows, int t, int tm, int tn,
                                                    int nstages_arg) {
  View v = *vp;
  v.b.uniform_idx = uniform_idx;
  const int nstages = NS > 0 ? NS : nstages_arg;
  __shared__ __attribute__((aligned(16))) float smem[C_STAGES * C_STAGE_FLOATS];
  const RamdShape &s = v.sh;
  const int L = blockIdx.x;
  const int xcd = L & 7, q = L >> 3;
  const int mt = q % tm, nt = (q / tm) * 8 + xcd; /* the m tiles of one W panel share an XCD */
  if (nt >= tn) return;
  const int m0 = mt * CM, n0 = 1 + nt * CN;       /* output columns start at 1 */
  // 8 waves: 0-3 multiply (one quarter of every K stage each), 4-7 only feed the LDS
  // ring.  An LDS-DMA instruction costs its issuing wave 100-200 cycles; on a wave of its
  // own that cost overlaps the other waves' MFMAs instead of delaying them.
  const int wave8 = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool loader = wave8 >= 4;
  const int wave = wave8 & 3;
  const int lm = lane & 31, kh = lane >> 5;
  const float *ehi_t = v.b.ehi + ((size_t)t * s.Scap + row0) * s.I;

  // --- LDS-DMA source addresses of this lane: 8 instructions per stage and wave.
  // Instruction i (0..31 over the workgroup) fills rows 2 (i & 15), +1 of A (i < 16) or B.
  const float *src[8];
  int kcol[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    int i = wave * 8 + j;
    int row = 2 * (i & 15) + (lane >> 5);
    int c = (lane & 31) ^ (row & 15); /* global chunk stored at this LDS position */
    const float *base;
    if (i < 16) {
      int r = m0 + row;
      base = ehi_t + (size_t)(r < nrows ? r : nrows - 1) * s.I;
    } else {
      int n = n0 + row;
      base = v.b.ih_w + (size_t)(n < s.I ? n : s.I - 1) * s.H;
    }
    src[j] = base + 1 + 4 * c; /* K runs over the hidden columns 1..hidden_size */
    kcol[j] = 1 + 4 * c;
  }
  // a stage whose 128 columns all lie inside K needs no per-chunk test
  auto issue_one = [&](int stage, int j) {
    float *dst = smem + (stage % C_STAGES) * C_STAGE_FLOATS + (wave * 8 + j) * 256;
    const int k0 = stage * CK;
    const float *g = src[j] + k0;
    /* last, partial stage only: chunks wholly past the hidden columns come from a zero line
     * (a chunk that straddles the end reads pad columns, which are zero in E) */
    if (k0 + CK > s.hidden_size) g = (k0 + kcol[j] <= s.hidden_size) ? g : v.b.zeros;
    __builtin_amdgcn_global_load_lds((glb_void_t *)g, (lds_void_t *)dst, 16, 0, 0);
  };
  auto issue = [&](int stage) {
    if (stage * CK + CK <= s.hidden_size) { /* a full stage: plain address arithmetic, nothing to select */
      float *dst = smem + (stage % C_STAGES) * C_STAGE_FLOATS + wave * 8 * 256;
#pragma unroll
      for (int j = 0; j < 8; j++)
        __builtin_amdgcn_global_load_lds((glb_void_t *)(src[j] + stage * CK), (lds_void_t *)(dst + j * 256), 16,
                                         0, 0);
      return;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) issue_one(stage, j);
  };

  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; i++) acc[i] = 0.0f;

  // --- what the epilogue needs from global memory (this thread's 4 output columns of one
  // row: the input values that gate them, and the operands of a short K tail) is fetched
  // now, so that its latency hides under the main loop
  const int etid = threadIdx.x & 255; /* epilogue work is done by the compute waves */
  const int erow_i = etid >> 3, ec4 = (etid & 7) * 4;
  const int er = m0 + erow_i < nrows ? m0 + erow_i : nrows - 1;
  const float *xrow = input_row<UNI>(v, row0 + er, t);
  float xin[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (loader) {
    /* the loaders' first stages go out before anything else in the workgroup touches memory */
#pragma unroll
    for (int p = 0; p < C_STAGES - 1; p++)
      if (p < nstages) issue(p);
  }
  // what the epilogue needs from global memory (the input values that gate this thread's four
  // outputs), requested by the compute waves now so that it has arrived by the end of the loop
  if (!loader) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      int n = n0 + ec4 + i;
      xin[i] = xrow[n <= s.hidden_size ? n : s.hidden_size];
    }
  }
  const uint32_t lds0 = lds_byte_addr(smem);
  const uint32_t rowoff = (uint32_t)lm * (CK * 4u);
  if (loader) {
    RING_LOADER_LOOP(C_STAGES, nstages, issue)
  } else {
    /* the K loop of a compute wave (k_ring.h): a stage's fragments are one quarter of its 32 chunks, on both operands */
    struct Frag { f32x4 a[4], b[4]; };
    auto rd = [&](int st, Frag &f) {
      const uint32_t abase = lds0 + (uint32_t)((st % C_STAGES) * C_STAGE_FLOATS) * 4u;
      const uint32_t bbase = abase + (uint32_t)(CM * CK) * 4u;
#pragma unroll
      for (int gi = 0; gi < 4; gi++) {
        int c = 2 * (4 * wave + gi) + kh;               /* chunk = 4 consecutive k */
        uint32_t off = rowoff + (uint32_t)((c ^ (lm & 15)) * 16);
        f.a[gi] = lds_read_b128(abase + off);
        f.b[gi] = lds_read_b128(bbase + off);
      }
    };
    auto multiply = [&](const Frag &f) {
#pragma unroll
      for (int gi = 0; gi < 4; gi++) mfma_k4(acc, f.a[gi], f.b[gi].x, f.b[gi].y, f.b[gi].z, f.b[gi].w);
    };
    auto step = [&](int st, Frag &f, Frag &fn) {
      /* every read issued so far has arrived: this stage's fragments are usable, and the
       * loaders may overwrite its buffer after the next barrier */
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (st + 1 < nstages) {
        __builtin_amdgcn_s_barrier(); /* stage st + 1 has landed */
        rd(st + 1, fn);
      }
      __builtin_amdgcn_sched_barrier(0);
      multiply(f);
      __builtin_amdgcn_sched_barrier(0);
    };
    if constexpr (NS > 0) {
      RING_READ_AHEAD(NS, Frag, rd, step)
    } else { /* any number of stages: read, wait, multiply, stage by stage (k_ring.h says why) */
      Frag f;
      for (int st = 0; st < nstages; st++) {
        __builtin_amdgcn_s_barrier(); /* stage st has landed */
        rd(st, f);
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(f.a[0]), "+v"(f.a[1]), "+v"(f.a[2]), "+v"(f.a[3]), "+v"(f.b[0]), "+v"(f.b[1]), "+v"(f.b[2]),
                       "+v"(f.b[3])
                     :
                     : "memory");
        multiply(f);
      }
    }
  }
  // --- sum the four waves' partial tiles through LDS.  The ring buffer that stage
  // `nstages` would have used holds stage nstages - 3, which every wave finished reading
  // two barriers ago and no DMA targets any more: it can be overwritten without a barrier.
  float *red = smem + (nstages % C_STAGES) * C_STAGE_FLOATS; /* [4][32][32] */
  if (!loader) {
#pragma unroll
    for (int g = 0; g < 16; g++) {
      int row = (g & 3) + 8 * (g >> 2) + 4 * kh;
      red[(wave * CM + row) * CN + lm] = acc[g];
    }
  }
  __syncthreads();
  if (loader) return;
  const int row = etid >> 3, c4 = (etid & 7) * 4;
  float e[4];
  {
    float4 p0 = ld4(red + (0 * CM + row) * CN + c4), p1 = ld4(red + (1 * CM + row) * CN + c4);
    float4 p2 = ld4(red + (2 * CM + row) * CN + c4), p3 = ld4(red + (3 * CM + row) * CN + c4);
    e[0] = (p0.x + p1.x) + (p2.x + p3.x);
    e[1] = (p0.y + p1.y) + (p2.y + p3.y);
    e[2] = (p0.z + p1.z) + (p2.z + p3.z);
    e[3] = (p0.w + p1.w) + (p2.w + p3.w);
  }
  const int r = m0 + row;
  float sq = 0.0f;
  if (r < nrows) {
    float *dst = v.b.ehi + ((size_t)(t + 1) * s.Scap + row0 + r) * s.I;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      int n = n0 + c4 + i;
      if (n <= s.hidden_size) {
        const float ev = act_backward(s, xin[i], e[i]);
        dst[n] = ev;
        sq += ev * ev;
      }
    }
  }
  sq += __shfl_xor(sq, 1, 64);
  sq += __shfl_xor(sq, 2, 64);
  sq += __shfl_xor(sq, 4, 64);
  if ((etid & 7) == 0 && r < nrows)
    v.b.esum_part[((size_t)t * (tn + 1) + nt) * s.Scap + row0 + r] = sq;
}

// ------------------------------------- BPTT chain step, 64 x 64 tiles (big sets) --
//
// The same step as k_chain_main for sets with many streams of a wide net (rnnca: 512 streams,
// hidden 2048), where the one-launch chain does not apply (its W panel would not fit the
// registers) and k_chain_main's 32 x 32 tiles are bound by the operand stream: a 32 x 32 tile
// moves 32 KB into LDS per 1024 MFMA cycles of a wave, 1024 workgroups x 512 KB = 512 MB of
// L2 -> LDS traffic per step.  Here the tile is 64 streams x 64 columns, the four multiplying
// waves own a 32 x 32 quadrant each over the WHOLE K (no split-K, no cross-wave reduction), and a
// K stage is 64 deep: 32 KB per 2048 MFMA cycles, half the bytes per MFMA, 256 workgroups = one
// per CU for 512 x 2048.  Staging is k_chain_main's: both operands K-contiguous, 16-byte chunk c
// of row r at position c ^ (r & 15) so that the b128 fragment reads are conflict free, four
// loader waves with LDS-DMA into a four-deep ring, fragments of stage st + 1 read while stage
// st multiplies (fully unrolled: NS stages).  Epilogue as in k_chain_main (zero-row mask, RESQRT
// derivative, store, per-tile sum of squares), one partial per 64 columns.
// Preconditions (launcher): every stream at one ring position, streams % 64 == 0,
// hidden_size == 64 * NS.
// MT = 32 (round 5): tiles of 32 streams for sets that leave the 64-stream grid short of the chip -- hidden 2048 with
// 256 streams is 4 x 32 = 128 tiles of 64 x 64 on 256 CUs, 0.48 of peak; as 32 x 64 tiles it is 256 -- with the K of
// every stage split over the two wave pairs instead (waves 0, 1: chunks 0 .. 7 of a stage's 16; waves 2, 3: 8 .. 15;
// both pairs a 32 x 32 quadrant each) and the two partial tiles added in the epilogue.  A stage is then 8 KB of A
// and 16 KB of B: six LDS-DMA instructions per loader wave.
template <int NS, int MT = 64>
__global__ __launch_bounds__(512) void k_chain_wide(const View *__restrict__ vp, int uniform_idx, int row0,
                                                    int nrows, int t, int tm, int tn) {
  constexpr bool HALF = MT == 32;
  constexpr int LPW = HALF ? 6 : 8; /* LDS-DMA instructions per loader wave and stage */
  extern __shared__ __attribute__((aligned(16))) float wsm[];
  View v = *vp;
  v.b.uniform_idx = uniform_idx;
  const RamdShape &s = v.sh;
  const int L = blockIdx.x;
  const int xcd = L & 7, q = L >> 3;
  const int mt = q % tm, nt = (q / tm) * 8 + xcd; /* the m tiles of one W panel share an XCD */
  if (nt >= tn) return;
  const int m0 = mt * MT, n0 = 1 + nt * WN; /* output columns start at 1 */
  const int wave8 = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool loader = wave8 >= 4;
  const int wave = wave8 & 3;
  const int lm = lane & 31, kh = lane >> 5;
  const float *ehi_t = v.b.ehi + ((size_t)t * s.Scap + row0) * s.I;
  const uint32_t lds0 = lds_byte_addr(wsm);

  if (loader) {
    // instruction i (0 .. 4 LPW - 1 over the four loader waves) fills four rows of the stage image -- the MT rows of A,
    // then the 64 of B: image row R = 4 i + (l >> 4) --: lane l brings chunk (l & 15) ^ (R & 15) of it
    const float *src[LPW];
#pragma unroll
    for (int j = 0; j < LPW; j++) {
      const int i = wave * LPW + j;
      const int R = 4 * i + (lane >> 4);
      const int c = (lane & 15) ^ (R & 15);
      const float *base = R < MT ? ehi_t + (size_t)(m0 + R) * s.I : v.b.ih_w + (size_t)(n0 + R - MT) * s.H;
      src[j] = base + 1 + 4 * c; /* K runs over the hidden columns 1..hidden_size */
    }
    auto issue = [&](int stage) {
      float *dst = wsm + (stage % W_STAGES) * W_STAGE_FLOATS + wave * LPW * 256;
#pragma unroll
      for (int j = 0; j < LPW; j++)
        __builtin_amdgcn_global_load_lds((glb_void_t *)(src[j] + stage * WK), (lds_void_t *)(dst + j * 256), 16, 0, 0);
    };
#pragma unroll
    for (int p = 0; p < W_STAGES - 1; p++)
      if (p < NS) issue(p);
#pragma unroll
    for (int st = 0; st < NS; st++) {
      const int ahead = (NS - 1 - st) < (W_STAGES - 2) ? (NS - 1 - st) : (W_STAGES - 2);
      if (ahead >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LPW) : "memory");
      else if (ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPW) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier(); /* stage st has landed; stage st - 1's buffer is free */
      if (st + W_STAGES - 1 < NS) issue(st + W_STAGES - 1);
    }
    __syncthreads();
    return;
  }

  // ------------------------------------------------------------------ multiply
  const int wm = wave >> 1, wn = wave & 1; /* HALF: wm is the wave pair's half of each stage's K */
  // the gate values of this thread's RPT x 4 outputs in the epilogue, requested now
  constexpr int RPT = MT / 16, NU = HALF ? 4 : 8; /* rows per thread; fragment pairs per stage and wave */
  const int etid = threadIdx.x; /* 0..255 */
  const int rq = etid >> 4, c4 = (etid & 15) * 4;
  float xin[RPT][4];
#pragma unroll
  for (int rr = 0; rr < RPT; rr++) {
    const float *xrow = input_row<true>(v, row0 + m0 + RPT * rq + rr, t) + n0 + c4;
#pragma unroll
    for (int i = 0; i < 4; i++) xin[rr][i] = xrow[i];
  }
  f32x16 acc; /* (a second accumulator taking turns with this one measured no difference) */
#pragma unroll
  for (int i = 0; i < 16; i++) acc[i] = 0.0f;
  const uint32_t arow = (uint32_t)((HALF ? 0 : wm * 32) + lm) * (WK * 4u), brow = (uint32_t)(MT + wn * 32 + lm) * (WK * 4u);
  struct Frag { f32x4 a[NU], b[NU]; };
  auto rd = [&](int st, Frag &f) {
    const uint32_t base = lds0 + (uint32_t)((st % W_STAGES) * W_STAGE_FLOATS) * 4u;
#pragma unroll
    for (int u = 0; u < NU; u++) {
      const uint32_t off = (uint32_t)(((2 * (u + (HALF ? NU * wm : 0)) + kh) ^ (lm & 15)) * 16);
      f.a[u] = lds_read_b128(base + arow + off);
      f.b[u] = lds_read_b128(base + brow + off);
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
    for (int u = 0; u < NU; u++) mfma_k4(acc, f.a[u], f.b[u].x, f.b[u].y, f.b[u].z, f.b[u].w);
    __builtin_amdgcn_sched_barrier(0);
  };
  RING_READ_AHEAD(NS, Frag, rd, step)
  // the tile through LDS (the ring buffer stage NS would have used was read four barriers ago); HALF: the two K
  // halves' tiles, [2][32][64], as rows 0 .. 31 and 32 .. 63 of the same image
  float *red = wsm + (NS % W_STAGES) * W_STAGE_FLOATS; /* [64][64] */
#pragma unroll
  for (int g = 0; g < 16; g++) {
    const int row = wm * 32 + (g & 3) + 8 * (g >> 2) + 4 * kh;
    red[row * WN + wn * 32 + lm] = acc[g];
  }
  __syncthreads();
  float *dst0 = v.b.ehi + ((size_t)(t + 1) * s.Scap + row0 + m0) * s.I + n0 + c4;
#pragma unroll
  for (int rr = 0; rr < RPT; rr++) {
    const int row = RPT * rq + rr;
    float4 e4 = ld4(red + row * WN + c4);
    if (HALF) {
      const float4 f4 = ld4(red + (32 + row) * WN + c4);
      add4(e4, f4);
    }
    const float e[4] = {e4.x, e4.y, e4.z, e4.w};
    float sq = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float ev = act_backward(s, xin[rr][i], e[i]);
      dst0[(size_t)row * s.I + i] = ev;
      sq += ev * ev;
    }
    sq += __shfl_xor(sq, 1, 64);
    sq += __shfl_xor(sq, 2, 64);
    sq += __shfl_xor(sq, 4, 64);
    sq += __shfl_xor(sq, 8, 64);
    if ((etid & 15) == 0) v.b.esum_part[((size_t)t * (tn + 1) + nt) * s.Scap + row0 + m0 + row] = sq;
  }
}
