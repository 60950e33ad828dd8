// k_delta_dma.h -- stage 4 of rnn_bptt_calc_deltas, one of its three forms: the weight-delta GEMM by LDS-DMA
// (recur-nn.c:343-358, 734-739), k_delta_dma with its ring's constants and the rest rows that ride along (DeltaRest).
// Included by kernels_bptt.hip alone (behind k_gemm.h: BK, GemmOut); launched by its launch_delta_dma for calc_delta_dma.
#pragma once
#include "k_common.h"
#include "k_gemm.h"
#include "k_ring.h"

// ------------------------------------------------ weight-delta GEMM by LDS-DMA --
//
// ih_delta[m][n] = sum over (step t, stream r) of X_t[r][m] * coef[t][r] * E_t[r][n]
// (recur-nn.c:343-358 for every executed step of every stream, with the stream's
// ih_scale folded in).  Both operands are K-major: a K tile is 32 streams of one step, a
// row of it 128 consecutive floats of a history slot (A) or of an error plane (B).
//
// Workgroup = 8 waves on one CU: waves 0-3 own a 64 x 64 quadrant of the 128 x 128 tile
// each (2 x 2 accumulators, 64 MFMAs per K tile and wave); waves 4-7 only move data:
// each K tile is 32 + 1 LDS-DMA wave instructions (16 KB of A, 16 KB of B, the tile's 32
// coefficients) into a four-deep ring, three tiles in flight.  One raw s_barrier per K
// tile; nothing else couples the two groups.  A K tile costs a compute wave 64 MFMAs
// (4096 cycles), so the barrier and the LDS read latency between tiles are a few per cent.
// The per-row coefficient is applied to the B fragments after the LDS read (select on
// zero: rows of steps a stream did not execute may hold anything).
//
// Preconditions (checked by the launcher, which otherwise uses k_gemm2): every stream at
// the same ring position, nrows % 32 == 0, hidden_size % 128 == 0, not RECLIP20.  Only
// whole 128-row tiles are computed here; the remaining rows (bias row 0 is in tile 0; the
// input rows above the last whole tile) go through the generic k_gemm with a row offset.
constexpr int DD_STAGES = 4;
constexpr int DD_STAGE_FLOATS = 2 * BK * 128 + 64; /* A, B, 32 coefficients (+ pad) */

/* The rows above the last whole 128-row tile (the input rows of a text net: 44 at the north
 * star) ride along: the tm workgroups that share a column tile and a K slice (mt = 0..tm-1;
 * eight at hidden 1024) each take every tm-th K tile of the slice, fetch the 32 x 64 piece of the history rows'
 * tail for it (columns rows_core .. rows_core + 63: past i_size they run into the next row,
 * which only feeds output rows nobody stores), and multiply it with the error fragments they
 * have in registers anyway: 8 more MFMAs per 16 in one K tile of tm, no second pass over
 * the error planes.  Their partial sums are plane z * tm + mt of `planes`. */
struct DeltaRest {
  float *planes;  /* [ks * tm][rows][ldc] */
  size_t stride;  /* floats between planes */
  int rows;       /* i_size - rows_core, <= RR */
  int col;        /* rows_core */
};
constexpr int DD_REST_FLOATS = BK * 128; /* the rest ring: two tiles of 32 k x 64 rows or one of 32 k x 128 */

#ifdef PC_STAMPS /* development builds only (tools/mkabl.sh -DPC_STAMPS, tools/gpu_delta_stamps.py) */
__device__ unsigned long long g_dd_stamps[64][8];
extern "C" void ramd_delta_stamps(unsigned long long *out) {
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dd_stamps), sizeof(unsigned long long) * 64 * 8));
}
#endif
/* RR: rows of the rest tile: 0 (none), 64 or 128 (a wave then has 32 or 64 rest rows x its 64 columns) */
template <int RR>
__global__ __launch_bounds__(512) void k_delta_dma(View v, int row0, int nrows, GemmOut o, DeltaRest dr) {
  /* above the noise generator's waves (priority 0), which share four SIMDs with workgroups of this launch while the set
   * has presynaptic noise: the launch runs at the pace of its slowest workgroup (multi-head step, 256 / 32 streams:
   * 369 -> 360 / 221 -> 218 us per generation; nothing else changes) */
  __builtin_amdgcn_s_setprio(2);
  extern __shared__ __attribute__((aligned(16))) float dsm[];
  const RamdShape &s = v.sh;
  const int L = blockIdx.x;
  // K slice z lives on 8 / ks XCDs (ks divides 8), so each XCD's L2 sees one slice of X
  // and E only; within a slice consecutive tiles alternate between its XCDs
  const int xcd = L & 7, q = L >> 3;
  const int per = 8 / o.ks;
  const int z = xcd / per, tile = q * per + (xcd % per);
  if (tile >= o.tm * o.tn) return;
  const int mt = tile / o.tn, nt = tile % o.tn;
  const int m0 = o.row0m + mt * 128, n0 = o.col0 + nt * 128; /* (row0m: a launch over the upper row tiles only) */
  const int kt0 = (int)(((long)o.nkt * z) / o.ks), kt1 = (int)(((long)o.nkt * (z + 1)) / o.ks);
  const int nst = kt1 - kt0;
  const int wave8 = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int rtiles = nrows / BK;
  /* stage st carries rest work when st % tm == mt; its tile sits in slot (st / tm) % 2 behind the
   * ring (tm >= 4, so a slot's previous tile was consumed long before the next one is fetched) */
  constexpr bool REST = RR > 0;
  constexpr int RI = RR / 64; /* 32-row groups of rest rows per wave */
  auto is_rest = [&](int st) { return REST && st < nst && st % o.tm == mt; };
  /* byte-free float offset of a stage's rest tile in the rest ring: two slots of 64 rows, one of 128 */
  auto rest_slot = [&](int st) { return RR == 64 ? ((st / o.tm) & 1) * (BK * 64) : 0; };
  float *const rest_ring = dsm + DD_STAGES * DD_STAGE_FLOATS;

  if (wave8 >= 4) {
    // ---------------------------------------------------------------- loaders
    const int w = wave8 - 4;
    // instruction i (0..31): rows 2 (i & 15), +1 of A (i < 16) or B; wave w issues i = 8 w + j
    /* Every DMA is (wave-uniform base, per-lane byte offset that never changes, wave-uniform
     * LDS address): issued as saddr + voffset by inline asm, a fetch costs the loader wave no
     * vector-ALU instruction -- beside a wave that issues f32 MFMAs back to back (they run on
     * the SIMD's vector ALU) such instructions wait for a gap in the MFMA stream. */
    const int ws = __builtin_amdgcn_readfirstlane(w);
    const unsigned voff = (unsigned)(((size_t)(lane >> 5) * s.I + (lane & 31) * 4) * sizeof(float));
    const unsigned voff_c = (unsigned)((lane & 31) * sizeof(float));
    const unsigned voff_r = RR == 128 ? voff : (unsigned)(((size_t)(lane >> 4) * s.I + (lane & 15) * 4) * sizeof(float));
    const uint32_t dsm_lds = __builtin_amdgcn_readfirstlane(lds_byte_addr(dsm));
    auto issue = [&](int st) {
      const int kt = kt0 + st;
      const int t = kt / rtiles, sb = (kt - t * rtiles) * BK;
      int slot = v.b.uniform_idx - t;
      if (slot < 0) slot += s.D;
      /* waves 0, 1 fetch the history rows (A), waves 2, 3 the error rows (B): rows 2 (i & 15), + 1 */
      const float *base = ws < 2 ? v.b.arena + ((size_t)slot * s.Scap + row0 + sb) * s.I + m0
                                 : v.b.ehi + ((size_t)t * s.Scap + row0 + sb) * s.I + n0;
      const uint32_t dst = dsm_lds + (uint32_t)(((st % DD_STAGES) * DD_STAGE_FLOATS + (ws < 2 ? 0 : BK * 128)) * sizeof(float));
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const int i15 = (ws & 1) * 8 + j; /* = (w * 8 + j) & 15 */
        lds_dma16(base + (size_t)(2 * i15) * s.I, voff, dst + (uint32_t)(i15 * 256 * sizeof(float)));
      }
      if (ws == 0) { /* the 32 coefficients of the tile: lanes 32-63 repeat them */
        lds_dma4(v.b.coef + (size_t)t * s.Scap + row0 + sb, voff_c,
                 dsm_lds + (uint32_t)(((st % DD_STAGES) * DD_STAGE_FLOATS + 2 * BK * 128) * sizeof(float)));
      }
      if (REST && ws == 3 && is_rest(st)) { /* the tail of the 32 history rows: four rows per instruction */
        const float *rb = v.b.arena + ((size_t)slot * s.Scap + row0 + sb) * s.I + dr.col;
        const uint32_t rdst = dsm_lds + (uint32_t)((DD_STAGES * DD_STAGE_FLOATS + rest_slot(st)) * sizeof(float));
        /* an instruction moves 1 KB: four rows of 64 floats or two of 128 */
#pragma unroll
        for (int j = 0; j < 8 * (RI ? RI : 1); j++)
          lds_dma16(rb + (size_t)((RR == 128 ? 2 : 4) * j) * s.I, voff_r, rdst + (uint32_t)(j * 256 * sizeof(float)));
      }
    };
#pragma unroll
    for (int p = 0; p < DD_STAGES - 1; p++)
      if (p < nst) issue(p);
    for (int st = 0; st < nst; st++) {
      // stages st+1 .. st+DD_STAGES-2 may stay in flight (8 or 9 DMAs per stage)
      const int ahead = min(DD_STAGES - 2, nst - 1 - st);
      if (w == 0) {
        if (ahead >= 2) asm volatile("s_waitcnt vmcnt(18)" ::: "memory");
        else if (ahead == 1) asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      } else if (REST && w == 3) {
        /* 8 (RR 64) or 16 (RR 128) more in flight for a rest stage among the ones ahead (at most one:
         * they are tm >= 4 apart) */
        const bool more = (ahead >= 1 && is_rest(st + 1)) || (ahead >= 2 && is_rest(st + 2));
        if (ahead >= 2) {
          if (more && RR == 128) asm volatile("s_waitcnt vmcnt(32)" ::: "memory");
          else if (more) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
          else asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
        } else if (ahead == 1) {
          if (more && RR == 128) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
          else if (more) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
          else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        } else {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
      } else {
        ring_wait_ahead(ahead);
      }
      __builtin_amdgcn_s_barrier(); /* stage st has landed; stage st-1's buffer is free */
      if (st + DD_STAGES - 1 < nst) issue(st + DD_STAGES - 1);
    }
    return;
  }

  // ------------------------------------------------------------------ compute
  const int wm = wave8 >> 1, wn = wave8 & 1;
  const int lm = lane & 31, kh = lane >> 5;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int g = 0; g < 16; g++) acc[i][j][g] = 0.0f;
  // The fragments of K group u + 1 (8 k: four MFMA steps of two k each) are read from LDS while the 16
  // MFMAs of group u are issued, ONE READ BEHIND EACH OF THE FIRST NINE MFMAs, and used after them.
  // This wave is the only one that feeds its SIMD's matrix pipe, and it issues in order: whatever stands
  // between the last MFMA of a group and the first of the next beyond the ~60 cycles of that MFMA's own
  // shadow is time the pipe idles.  Measured (round 3, ablation builds): the nine reads bunched in front of
  // a group cost 3.8 us of a 100 us launch, the eight coefficient multiplies 4.4 us, and a run-time test
  // that skipped the multiplies cost what they did.  So: reads spread one per MFMA shadow; inline asm
  // (`ds_read2st64_b32`: two k rows, 128 floats apart, per instruction; immediate offsets in units of 64
  // floats reach every k of a stage; four address registers per STAGE) because as plain loads hipcc waited
  // for them twice per K tile; the multiplies only for a stage whose coefficients are not all exactly 1.0
  // (out of line); the stage's rest-row bookkeeping as two counters instead of a division per stage.
  struct Frag {
    f32x2 a[2][2], e[2][2]; /* [i or jn][k pair]: k = 8 g + 4 kh + 2 pair, + 1 */
    f32x4 cf;
    f32x2 ar[RI ? RI : 1][2]; /* rest rows (REST stages only) */
  };
  f32x16 racc[RI ? RI : 1][2];
#pragma unroll
  for (int i = 0; i < (RI ? RI : 1); i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int g = 0; g < 16; g++) racc[i][j][g] = 0.0f;
  /* per-lane byte addresses within a stage: A rows i = 0, 1; E columns jn = 0, 1; the coefficients (four of the
   * group for the multiplies; the lane's one of the stage's 32 for the all-ones test); the rest rows */
  const uint32_t dsm0 = lds_byte_addr(dsm);
  const uint32_t la_lane = dsm0 + 4u * (uint32_t)(4 * kh * 128 + wm * 64 + lm);
  const uint32_t le_lane = dsm0 + 4u * (uint32_t)(BK * 128 + 4 * kh * 128 + wn * 64 + lm);
  const uint32_t lc_lane = dsm0 + 4u * (uint32_t)(2 * BK * 128 + 4 * kh);
  const uint32_t lf_lane = dsm0 + 4u * (uint32_t)(2 * BK * 128 + (lane & 31));
  const uint32_t lr_lane = lds_byte_addr(rest_ring) + 4u * (uint32_t)(4 * kh * RR + wm * (RR / 2) + lm);
  uint32_t ad_a0 = 0, ad_a1 = 0, ad_e0 = 0, ad_e1 = 0, ad_c = 0, ad_r = 0; /* of the stage being READ */
  float cfl = 0.0f; /* the lane's coefficient of that stage */
  /* `slot`: the stage's ring buffer (st % DD_STAGES); `par`: which half of the rest ring ((st / tm) & 1) */
  auto stage_addr = [&](int slot, bool rest, int par) {
    const uint32_t sb = (uint32_t)(slot * DD_STAGE_FLOATS * (int)sizeof(float));
    ad_a0 = la_lane + sb;
    ad_a1 = ad_a0 + 128u;
    ad_e0 = le_lane + sb;
    ad_e1 = ad_e0 + 128u;
    ad_c = lc_lane + sb;
    if (REST && rest) ad_r = lr_lane + (uint32_t)((RR == 64 ? par * (BK * 64) : 0) * (int)sizeof(float));
    cfl = lds_read_b32_off<0>(lf_lane + sb);
  };
  /* read k (0 .. 8) of group G of the stage whose addresses are set */
  auto rd1 = [&](auto GC, auto KC, Frag &f) {
    constexpr int G = decltype(GC)::value, k = decltype(KC)::value;
    if constexpr (k == 0) {
      f.cf = lds_read_b128_off<32 * G>(ad_c);
    } else {
      constexpr int pair = (k - 1) >> 2, which = (k - 1) & 3;
      constexpr int o0 = 2 * (8 * G + 2 * pair), o1 = o0 + 2;
      if constexpr (which == 0) f.a[0][pair] = lds_read2st64<o0, o1>(ad_a0);
      if constexpr (which == 1) f.e[0][pair] = lds_read2st64<o0, o1>(ad_e0);
      if constexpr (which == 2) f.a[1][pair] = lds_read2st64<o0, o1>(ad_a1);
      if constexpr (which == 3) f.e[1][pair] = lds_read2st64<o0, o1>(ad_e1);
    }
  };
  /* ... and the rest rows' 2 RI reads of that group (rest stages only) */
  auto rd_rest = [&](auto GC, Frag &f) {
    constexpr int G = decltype(GC)::value;
    constexpr int RU = RR ? RR / 64 : 1; /* k rows of the rest tile are RR floats apart: RR / 64 offset units */
#pragma unroll
    for (int i = 0; i < RI; i++) {
      f.ar[i][0] = lds_read2st64<(8 * G + 0) * RU, (8 * G + 1) * RU>(ad_r + 128u * (uint32_t)i);
      f.ar[i][1] = lds_read2st64<(8 * G + 2) * RU, (8 * G + 3) * RU>(ad_r + 128u * (uint32_t)i);
    }
  };
  /* One group: the MFMAs on `cur` (whose reads were issued during the group before: all landed), the reads
   * of group GN into `nxt` behind the first nine of them.
   * `ones`: every coefficient of the stage is exactly 1.0 (the usual case: no stream was soft-clipped, none
   * broke off early) -- the error fragments go into the MFMAs as they are. */
  /* (the flags are ints in scalar registers: as bools that live across blocks hipcc keeps them as vector
   * masks and rebuilds each with two vector-ALU instructions per use) */
  auto group = [&](auto GN, Frag &cur, Frag &nxt, int rest, int rest_next, int ones) {
    frag_wait<0>(cur.cf, cur.a, cur.e);
    /* v_mul_legacy_f32: 0 * x is 0 for ANY x (a step past the break may hold inf), otherwise the
     * IEEE product: select and multiply in one instruction of the MFMAs' own ALU.  In place, all eight
     * in ONE statement: as separate statements with outputs of their own hipcc recycled two registers
     * between the MFMAs, and results went wrong.  (One MFMA sequence behind a conditional multiply, not
     * two sequences: with the MFMAs in both arms hipcc copies accumulators at the join.) */
    if (__builtin_expect(ones == 0, 0))
      asm volatile("v_mul_legacy_f32 %0, %8, %0\n\tv_mul_legacy_f32 %1, %9, %1\n\t"
                   "v_mul_legacy_f32 %2, %10, %2\n\tv_mul_legacy_f32 %3, %11, %3\n\t"
                   "v_mul_legacy_f32 %4, %8, %4\n\tv_mul_legacy_f32 %5, %9, %5\n\t"
                   "v_mul_legacy_f32 %6, %10, %6\n\tv_mul_legacy_f32 %7, %11, %7\n\ts_nop 1"
                   : "+v"(cur.e[0][0][0]), "+v"(cur.e[0][0][1]), "+v"(cur.e[0][1][0]), "+v"(cur.e[0][1][1]),
                     "+v"(cur.e[1][0][0]), "+v"(cur.e[1][0][1]), "+v"(cur.e[1][1][0]), "+v"(cur.e[1][1][1])
                   : "v"(cur.cf[0]), "v"(cur.cf[1]), "v"(cur.cf[2]), "v"(cur.cf[3]));
    if (REST && __builtin_expect(rest_next != 0, 0)) rd_rest(GN, nxt); /* wave-uniform */
    __builtin_amdgcn_sched_barrier(0);
    static_for<16>([&](auto MC) {
      constexpr int m = decltype(MC)::value, jj = m >> 2, i = (m >> 1) & 1, jn = m & 1;
      acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a[i][jj >> 1][jj & 1], cur.e[jn][jj >> 1][jj & 1], acc[i][jn], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (m < 9) {
        rd1(GN, std::integral_constant<int, m>{}, nxt);
        __builtin_amdgcn_sched_barrier(0);
      }
    });
    if (REST && __builtin_expect(rest != 0, 0)) { /* wave-uniform: this wave's 32 or 64 rest rows x its 64 columns */
#pragma unroll
      for (int jj = 0; jj < 4; jj++)
#pragma unroll
        for (int i = 0; i < RI; i++)
#pragma unroll
          for (int jn = 0; jn < 2; jn++)
            racc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.ar[i][jj >> 1][jj & 1], cur.e[jn][jj >> 1][jj & 1], racc[i][jn], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  /* (the lane's coefficient was requested before the nine reads of the stage's group 0) */
  auto all_ones = [&]() {
    asm volatile("s_waitcnt lgkmcnt(9)" : "+v"(cfl));
    return __builtin_amdgcn_readfirstlane(__ballot(cfl == 1.0f) == ~0ull ? 1 : 0);
  };
  Frag f0, f1;
  /* stage st carries rest work when st % tm == mt (ph), in half (st / tm) & 1 of the rest ring (par) */
  int ph = 0, par = 0;
#ifdef PC_STAMPS
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    g_dd_stamps[0][4] = __builtin_amdgcn_s_memrealtime();
    g_dd_stamps[0][7] = __builtin_readcyclecounter(); /* shader clocks: with [1][7], the clock the loop ran at */
  }
#endif
  if (nst > 0) {
    __builtin_amdgcn_s_barrier(); /* stage 0 has landed */
    asm volatile("" ::: "memory");
    stage_addr(0, REST && mt == 0, 0);
    if (REST && mt == 0) rd_rest(std::integral_constant<int, 0>{}, f0);
    static_for<9>([&](auto KC) { rd1(std::integral_constant<int, 0>{}, KC, f0); });
  }
  int ones = all_ones();
  for (int st = 0; st < nst; st++) {
    const int r = __builtin_amdgcn_readfirstlane(REST && ph == mt ? 1 : 0);
    int phn = ph + 1, parn = par;
    if (phn == o.tm) {
      phn = 0;
      parn ^= 1;
    }
    const bool more = st + 1 < nst;
    const int rn = __builtin_amdgcn_readfirstlane(REST && more && phn == mt ? 1 : 0);
    group(std::integral_constant<int, 1>{}, f0, f1, r, r, ones);
    group(std::integral_constant<int, 2>{}, f1, f0, r, r, ones);
    group(std::integral_constant<int, 3>{}, f0, f1, r, r, ones);
    /* group 3 runs across the stage boundary: its reads are group 0 of stage st + 1 (after the last stage
     * group 0 of the same stage once more, into the idle fragment: every group then looks the same) */
    if (more) {
#ifdef PC_STAMPS
      if (blockIdx.x == 0 && threadIdx.x == 0 && st < 63) g_dd_stamps[st + 1][4] = __builtin_amdgcn_s_memrealtime();
#endif
      __builtin_amdgcn_s_barrier(); /* stage st + 1 has landed; stage st - 1's buffer is free */
      asm volatile("" ::: "memory");
#ifdef PC_STAMPS
      if (blockIdx.x == 0 && threadIdx.x == 0 && st < 63) g_dd_stamps[st + 1][5] = __builtin_amdgcn_s_memrealtime();
#endif
      stage_addr((st + 1) % DD_STAGES, rn != 0, parn);
    }
    group(std::integral_constant<int, 0>{}, f1, f0, r, rn, ones);
#ifdef PC_STAMPS
    if (blockIdx.x == 0 && threadIdx.x == 0 && st < 63) g_dd_stamps[st][3] = ones ? 1ull : 0ull;
#endif
    if (more) ones = all_ones();
    ph = phn;
    par = parn;
  }
#ifdef PC_STAMPS
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    g_dd_stamps[0][6] = __builtin_amdgcn_s_memrealtime();
    g_dd_stamps[1][7] = __builtin_readcyclecounter();
  }
#endif
  float *c = o.slab + (size_t)z * o.zs;
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int jn = 0; jn < 2; jn++) {
      const int col = n0 + wn * 64 + jn * 32 + lm;
#pragma unroll
      for (int g = 0; g < 16; g++) {
        int row = m0 + wm * 64 + i * 32 + (g & 3) + 8 * (g >> 2) + 4 * kh;
        c[(size_t)row * o.ldc + col] = acc[i][jn][g];
      }
    }
  if (REST) {
    float *rp = dr.planes + (size_t)(z * o.tm + mt) * dr.stride;
#pragma unroll
    for (int i = 0; i < RI; i++)
#pragma unroll
      for (int jn = 0; jn < 2; jn++) {
        const int col = n0 + wn * 64 + jn * 32 + lm;
#pragma unroll
        for (int g = 0; g < 16; g++) {
          int row = wm * (RR / 2) + i * 32 + (g & 3) + 8 * (g >> 2) + 4 * kh;
          if (row < dr.rows) rp[(size_t)row * o.ldc + col] = racc[i][jn][g];
        }
      }
  }
}

