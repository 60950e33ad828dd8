// k_fwd_top.h -- the text step's forward pass and top layer as one launch: k_fwd_top, over fwd_fused_tile (k_fwd_fused.h)
// and text_top2_rest (k_text_top2.h).  kernels_forward.hip launches it (launch_fwd_top) and keeps its process state.
#pragma once
#include "k_coop.h"
#include "fwd_top_plan.h"
#include "k_fwd_fused.h"
#include "k_text_top2.h"
// ------------------------------------ the text step's forward pass AND top layer in one launch --
//
// k_fwd_fused + k_text_top2 as one launch (fwd_top_plan.h says when): between the two launches lie 1.7 us of boundary, and
// k_text_top2 spends its first 3.5 us waiting for its rows of W_ho, which depend on nothing the forward pass computes.
// 256 workgroups of sixteen waves, one per CU (113 KB of LDS, 1024 threads); the workgroup on seat j of XCD g (the
// residency probe's seat table, as in k_chain_persist: k_coop.h; DESIGN.md, "Launches whose workgroups wait for one
// another") is column tile j of row tile g:
//   phase 1: waves 0-7 run fwd_fused_tile, k_fwd_fused's work for the tile.  Waves 8-15 request their rows of W_ho as the
//            kernel's first instructions and then only keep the barrier count; waves 4-7, the loaders, request theirs when
//            their last stage has been taken (their counted vmcnt waits see nothing of it), waves 0-3 behind the hand-off;
//   hand-off: the block's stores drained, a barrier, ONE plain store of the launch's number into the workgroup's flag
//            word -- row tile and readers share the XCD's L2, the chain's protocol.  Wave 8 polls the row tile's 32 flags
//            past the L1, bounded: a time-out or the abort word set ends the workgroup and raises the abort word
//            (host-mapped: ramd_dsync reports it), and lowers the workgroup's own flag so that no late workgroup of the row
//            tile goes on alone;
//   phase 2: text_top2_rest for stream j of the row tile, all sixteen waves, the sums and the target read past the L1,
//            the ring's LDS for its hidden row and column sums.
// A workgroup on an XCD past the set's row tiles has nothing to do.
struct FwdTopSync {
  unsigned flags[FWD_TOP_MAX_TILES][32]; /* [row tile][column tile]: the number of the last launch that stored its block */
  unsigned abort;                        /* raised by any workgroup that gives up */
};
#if defined(PC_STAMPS) || defined(FT_STAMPS) /* development builds only: workgroup (0, 0)'s phases (-DFT_STAMPS: these stamps alone) */
__device__ unsigned long long g_ft_stamps[8];
extern "C" void ramd_fwd_top_stamps(unsigned long long *out) {
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ft_stamps), sizeof(unsigned long long) * 8));
}
#define FT_STAMP(i) do { if (g == 0 && j == 0 && threadIdx.x == ((i) < 4 ? 0u : 512u)) g_ft_stamps[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define FT_STAMP(i) do { } while (0)
#endif
template <int NS>
__global__ __launch_bounds__(1024) void k_fwd_top(const View *__restrict__ vp, int new_idx, int row0, int nrows, int text_i,
                                                  int global_first, int n_set, FwdTopSync *sy, unsigned seq,
                                                  unsigned *host_abort, const unsigned *seats) {
  /* (first: one scalar load beside the arguments' -- k_coop.h: seat_tbl_p) */
  const unsigned hw_xcc = coop_hw_xcc();
  const unsigned seat = coop_seat(seats, hw_xcc);
  __shared__ __attribute__((aligned(16))) float smem[C_STAGES * C_STAGE_FLOATS];
  __shared__ unsigned ft_dead;
  BND_MARK(g_bnd_fwd, 0);
  View v = *vp;
  const int wave8 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int g = (int)hw_xcc, j = (int)seat;
  if (seat >= 32u) { /* a CU the probe did not name: cannot happen with one workgroup per CU on a 256-CU part */
    if (threadIdx.x == 0) coop_give_up(&sy->abort, host_abort, COOP_ABORT_FWD_TOP);
    return;
  }
  if (g >= nrows / CM) return;
  FT_STAMP(0);
  unsigned *const flag = &sy->flags[g][j];
  float4 wv[T2_NB];
  if (wave8 >= 8) {
    text_top2_request(v, wv);
    /* fwd_fused_tile's barriers (NS and its __syncthreads), and the hand-off's */
#pragma unroll
    for (int i = 0; i < NS + 2; i++) __builtin_amdgcn_s_barrier();
  } else {
    fwd_fused_tile<NS, RAMD_IN_TEXT, true>(v, smem, g, j, new_idx, row0, nrows, FWD_TOP_HIDDEN / CN, NS, RAMD_IN_TEXT, text_i,
                                     global_first, n_set, nullptr, 0);
    if (wave8 >= 4) text_top2_request(v, wv);
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); /* the block of sums, the partials, the slot, index and target: in the L2 */
    FT_STAMP(1);
    __builtin_amdgcn_s_barrier();
    if (threadIdx.x == 0) *flag = seq; /* plain: stays in this XCD's L2, where the row tile's polls find it */
    if (wave8 < 4) text_top2_request(v, wv);
    FT_STAMP(2);
  }
  // ---- every column tile of the row tile has stored its block?  (wave 8: it requested its W_ho rows as the kernel's first
  // instructions, the K loop ago.  The poll's vmcnt(0) waits for them too, loads return in order: after 8 stages that is
  // no wait; it is never wrong, and the rows are needed right behind the poll anyway.  Waves 0-7 asked later.)
  if (wave8 == 8) {
    const unsigned *fbase = &sy->flags[g][0];
    const unsigned poll_off = (unsigned)((lane & 31) * sizeof(unsigned));
    /* has somebody else given up; have we been here for a second */
    const unsigned dead = coop_poll(fbase, poll_off, seq, &sy->abort) ? 0u : 1u;
    if (dead && lane == 0) {
      coop_give_up(&sy->abort, host_abort, COOP_ABORT_FWD_TOP);
      __hip_atomic_store(flag, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); /* (no late workgroup of the row tile goes on alone) */
    }
    if (lane == 0) ft_dead = dead;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();
  {
    unsigned dead;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(dead) : "v"(lds_byte_addr(&ft_dead)) : "memory");
    if (__builtin_amdgcn_readfirstlane(dead)) return;
  }
  FT_STAMP(4);
  const int jc = g * CM + j, r = row0 + jc; /* the stream: within the call, state row */
  text_top2_rest<true, true>(v, jc, r, nrows, -(FWD_TOP_HIDDEN / CN), smem, wv);
  FT_STAMP(5);
  BND_MARK(g_bnd_fwd, 1);
}
