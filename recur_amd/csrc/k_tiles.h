// k_tiles.h -- the tile sizes that both the kernels and the launchers' planning (calc_plan.h, chain_plan.h, fwd_plan.h) read, and the split-K
// rule.  No HIP here: the host compiler alone can include it.
#pragma once
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>

constexpr int CM = 32, CN = 32, CK = 128; /* the BPTT chain's tile (k_common.h) */
constexpr int BM = 64, BN = 64, BK = 32;  /* k_gemm (k_gemm.h) */
constexpr int BM2 = 128, BN2 = 128;       /* k_gemm2 */
constexpr int RAMD_MAX_REST_PLANES = 64;
constexpr int THP_ROWS = 128;   /* k_top_heads_partial: rows of W_ho per workgroup */
constexpr int XD_NT = 3;        /* k_extras_dense: column tiles of 16 */
constexpr int DD_FLAG_LOADS = 8; /* k_delta_direct: 4 x 256 streams of n_exec, of ih_scale */
constexpr int OUT_SEGS = 16;    /* segments of the hidden row in the output-layer kernels (k_out_layer, k_text_top) */
/* 64 x 64 tiles of the wide chain step and the wide forward GEMM (k_chain_wide, k_fwd_wide) */
constexpr int WM = 64, WN = 64, WK = 64, W_STAGES = 4;
constexpr int W_STAGE_FLOATS = (WM + WN) * WK; /* 32 KB */
/* the one-launch chain (k_chain_persist.h): streams per sub-chain, its partial-tile area, its LDS per workgroup at hidden
 * size K -- more than half a CU's, so one workgroup per CU; the residency probe (kernels_coop.hip) has the same footprint */
constexpr int PC_SUB = 16;
constexpr int PC_RED_FLOATS = 4 * PC_SUB * 32;
constexpr int pc_lds_bytes(int K) { return (2 * PC_SUB * K + 2 * PC_RED_FLOATS) * 4 + 64; }
/* the K blocks (8 MFMAs each) that its early form issues under the row stores' drain (k_chain_persist.h, EARLY, beside the two
 * constants tuned to it): chain_plan.h hands the number to the launcher, which has that one instantiation */
#ifndef PC_EARLY
#define PC_EARLY 1
#endif
constexpr int FF_MAXIN = 64;    /* k_fwd_fused: dense input columns at most */
constexpr int T2_NB = 17;       /* k_text_top2 (k_text_top2.h): float4 of W_ho per lane, i.e. a wave's rows in one batch of 4 x T2_NB */
/* ... and the LDS its body needs, in floats: [H] hidden row, [16 waves][O] column sums, [O] outputs, [O] output error */
constexpr int text_top2_lds_floats(int H, int O) { return H + 18 * O; }

/* the RECUR_AMD_* switches, which the plans read: kernels_support.hip in the library (k_common.h declares it hidden there,
 * the version script keeps it unexported); the plans' test harnesses have their own */
int env_int(const char *name, int dflt);

// Split-K factor: enough workgroups to give every CU two or three, without
// shredding K into single tiles.
static inline int pick_ks(int tiles, int nkt, size_t slab_floats, size_t out_floats) {
  const int cus = 256;
  double best = 1e30;
  int ks = 1;
  for (int k = 1; k <= 16 && k <= nkt; k++) {
    long wgs = (long)tiles * k;
    /* CUs run up to ~3 of these workgroups side by side; count time in
     * "K tiles on the busiest CU" plus a fill/drain charge per workgroup */
    double per_cu = (double)((wgs + cus - 1) / cus);
    double cost = per_cu * ((double)nkt / k) + 2.0 * (per_cu > 3 ? per_cu / 3 : 1) + 0.15 * k;
    if (cost < best) {
      best = cost;
      ks = k;
    }
  }
  if (ks > nkt) ks = nkt;
  if (ks < 1) ks = 1;
  while (ks > 1 && (size_t)ks * out_floats > slab_floats) ks--;
  if (out_floats > slab_floats) { /* the workspace is sized for every output at engine creation */
    fprintf(stderr, "librecur_amd: a GEMM output of %zu floats does not fit the split-K workspace (%zu)\n",
            out_floats, slab_floats);
    abort();
  }
  return ks;
}
