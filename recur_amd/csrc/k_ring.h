// k_ring.h -- the K loop over an LDS operand ring, stated once for the kernels that run it: k_chain_main (k_chain_steps.h),
// k_fwd_wide (k_fwd_wide.h) and fwd_fused_tile (k_fwd_fused.h) whole, k_chain_wide and k_delta_dma's loaders in part.
//
// A workgroup's loader waves bring operand stages global -> LDS by LDS-DMA into a ring of STAGES buffers, eight DMA
// instructions per stage and loader wave; its compute waves multiply one stage while the fragments of the next are on
// their way from LDS.  One raw s_barrier per stage is the whole protocol ("The operand ring's K loop").
#pragma once
#include "k_common.h"

/* The loader's counted wait in front of barrier st: the `ahead` stages behind stage st that have been issued may stay in
 * flight, eight DMA instructions each (loads return in order; vmcnt counts instructions).  A ring keeps at most two. */
__device__ __forceinline__ void ring_wait_ahead(int ahead) {
  if (ahead >= 2) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  else if (ahead == 1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

/* A loader wave's loop, behind its issue of stages 0 .. STAGES - 2: wait, barrier, issue ahead.  issue(stage): the kernel's.
 * (This and RING_READ_AHEAD are macros and not function templates: hipcc optimises a function template on its own before it
 * inlines it -- unrolls its loop without knowing the lambda, or the number of stages -- and the kernels then keep neither the
 * instructions nor the registers of the loop written in place; profiles/NOTES_r19.md.  Both are brace blocks: a statement.) */
#define RING_LOADER_LOOP(STAGES, nstages, issue)                                                  \
  { _Pragma("unroll") for (int st_ = 0, n_ = (nstages); st_ < n_; st_++) {                        \
    ring_wait_ahead(min((STAGES) - 2, n_ - 1 - st_));                                              \
    __builtin_amdgcn_s_barrier(); /* stage st_ has landed; stage st_ - 1's buffer is free */       \
    if (st_ + (STAGES) - 1 < n_) issue(st_ + (STAGES) - 1);                                        \
  } }

/* The four MFMAs of one chunk of four consecutive k: a = the lane's row of A at those k, b0 .. b3 its column of B. */
__device__ __forceinline__ void mfma_k4(f32x16 &acc, const f32x4 &a, float b0, float b1, float b2, float b3) {
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b2, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b3, acc, 0, 0, 0);
}

/* A compute wave's loop over NS stages, one stage behind its own LDS reads.  Frag: the kernel's struct of one stage's
 * fragments (two take turns); rd(st, f) requests stage st's into f with inline-asm ds_reads; step(st, f, fn) waits for all
 * requested so far (lgkmcnt(0)), passes the barrier of stage st + 1 and requests its fragments into fn where there is
 * one, then multiplies f between two sched_barriers: neither ds_read latency nor barrier between two blocks of MFMAs.
 * ONLY FULLY UNROLLED (NS a compile-time constant): in a rolled loop the compiler may copy the ping-pong fragment
 * registers right after the ds_read that fills them -- before the data has arrived -- since it cannot see that an
 * inline-asm load completes later.  A kernel that also takes any number of stages keeps a rolled form of its own without
 * read-ahead: barrier, rd, an s_waitcnt lgkmcnt(0) that names the fragment's registers as "+v", multiply. */
#define RING_READ_AHEAD(NS, Frag, rd, step)                                  \
  {                                                                          \
    static_assert((NS) > 0, "fully unrolled only");                          \
    Frag f0_, f1_;                                                           \
    __builtin_amdgcn_s_barrier(); /* stage 0 has landed */                   \
    rd(0, f0_);                                                              \
    _Pragma("unroll") for (int st_ = 0; st_ < (NS); st_ += 2) {              \
      step(st_, f0_, f1_);                                                   \
      if (st_ + 1 < (NS)) step(st_ + 1, f1_, f0_);                           \
    }                                                                        \
  }
