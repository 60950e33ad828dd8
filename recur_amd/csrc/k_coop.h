// k_coop.h -- the device part of the one-per-CU launches' protocol ("Launches whose workgroups wait for one
// another"; the pure part: coop_rule.h, the process state: kernels_coop.hip), for the kernels whose 256 workgroups wait
// for one another through flags in an XCD's L2: k_chain_persist (k_chain_persist.h) and k_fwd_top (k_fwd_top.h).
// Where a workgroup is (XCD, CU) and which seat that gives it; the bounded poll; the give-up pair.
#pragma once
#include "k_common.h"
#include "coop_rule.h"

typedef __attribute__((address_space(1))) unsigned gu32;

// ---- process state (kernels_coop.hip) ----
/* the residency probe's answer, made at the first call that asks (a launch and a wait, once per process) */
RAMD_LOCAL SeatRule coop_seat_rule(hipStream_t st);
/* a launch gave up and its caller goes on (the chain's checked mode): the abort word cleared, no further launch of
 * this kind in the process */
RAMD_LOCAL void coop_mark_broken(void);

// ---- where am I ----
/* HW_REG_XCC_ID (register 20) bits 0 .. 3: the XCD this wave runs on */
__device__ __forceinline__ unsigned coop_hw_xcc() { return __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 7u; }
/* HW_REG_HW_ID (register 4) bits 8 .. 15: cu_id[3:0], sh_id, se_id[2:0] -- the CU's number within its XCD */
#define PC_HW_CU_KEY() (__builtin_amdgcn_s_getreg(((8 - 1) << 11) | (8 << 6) | 4) & 0xffu)
/* The seat table (coop_rule.h: SeatTable) is read through a CONSTANT-address-space pointer as the kernel's first
 * instructions: one scalar load beside the loads of the arguments and of the View.  (As a plain global pointer, and as a
 * by-value argument, hipcc made it a vector load behind everything else: +1.3 us per generation of the chain.) */
typedef const __attribute__((address_space(4))) unsigned *seat_tbl_p;
/* the seat of the CU this workgroup runs on (one workgroup per CU), >= 32: a CU the probe did not name */
__device__ __forceinline__ unsigned coop_seat(const unsigned *seats, unsigned xcc) {
  return ((seat_tbl_p)seats)[xcc * (unsigned)COOP_CU_KEYS + PC_HW_CU_KEY()];
}

// ---- the bounded poll ----
#ifndef PC_SLEEP1
#define PC_SLEEP1 1 /* s_sleep units (64 cycles) between two polls */
#endif
constexpr unsigned COOP_ALARM_PERIOD = 1024;  /* polls between two looks at the abort word */
constexpr unsigned COOP_POLL_BOUND = 1u << 21; /* polls before giving up: ~1 s -- a co-tenant's long kernel may hold CUs for a while */
/* Wait until the flag words at fbase + lane_off (fbase wave-uniform, one word per lane) are all >= want: true.  One
 * L1-bypassing (`sc1`) vector load per lane and ONE v_cmp per poll: beside a wave that issues f32 MFMAs back to back a
 * polling wave gets no more than that through (k_chain_persist.h: wait_for).  Flags compare as unsigned numbers
 * (coop_rule.h: the launcher starts the sequence over long before it wraps).  Rarely -- every COOP_ALARM_PERIOD polls --
 * it looks at the sync block's abort word: false when somebody has given up, or after COOP_POLL_BOUND polls.  That bound
 * is what makes a hang impossible.  What a caller does about a false (raise the alarm itself, or only heed it) is its
 * own: it tests the answer, or, where it has nothing else to do with it, hands the give-up in as `on_give_up`, which
 * runs at that moment.  (The two compile differently around the call, which is all that tells them apart:
 * profiles/NOTES_r18.md, "the compiled kernels".) */
struct CoopHeedOnly { __device__ void operator()() const {} };
template <class F = CoopHeedOnly>
__device__ __forceinline__ bool coop_poll(const void *fbase, unsigned lane_off, unsigned want, const unsigned *abort_word,
                                          F on_give_up = F{}) {
  bool seen = true;
  for (unsigned spins = 0;; spins++) {
    unsigned got;
    asm volatile("global_load_dword %0, %1, %2 sc1\n\ts_waitcnt vmcnt(0)" : "=v"(got) : "v"(lane_off), "s"(fbase) : "memory");
    if (__all(got >= want)) break;
    if ((spins & (COOP_ALARM_PERIOD - 1u)) == COOP_ALARM_PERIOD - 1u) {
      const unsigned ab = __hip_atomic_load((const gu32 *)abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (__any(ab != 0u) || spins > COOP_POLL_BOUND) {
        on_give_up();
        seen = false;
        break;
      }
    }
    __builtin_amdgcn_s_sleep(PC_SLEEP1);
  }
  return seen;
}

// ---- giving up ----
/* One lane of a workgroup that gives up: the sync block's abort word, which every poll of the launch heeds, and the
 * host-mapped word with the reason (coop_rule.h: CoopAbort), which ramd_dsync reads at the next synchronisation and
 * aborts on -- results are never silently wrong. */
__device__ __forceinline__ void coop_give_up(unsigned *abort_word, unsigned *host_abort, unsigned code) {
  __hip_atomic_store((gu32 *)abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(host_abort, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
