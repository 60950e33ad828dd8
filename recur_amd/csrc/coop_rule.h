// coop_rule.h -- the pure part of the one-per-CU launches' protocol ("Launches whose workgroups wait for one
// another"): the abort codes, what the residency probe's answer means (resident, dealt in turn, the seat table), the
// seat mode of a chain launch, and when a flag sequence starts over.  The device part is k_coop.h, the process state
// kernels_coop.hip.  No HIP call and no pointer followed: C (engine.c) and C++ include it with the host compiler alone,
// and tests/test_coop_rule.py asks it on a machine without a GPU.
#pragma once
#include <assert.h>
#include <string.h>

/* what a workgroup that gives up writes into the host-mapped abort word; ramd_dsync (engine.c) turns it into a message
 * and an abort() */
enum CoopAbort {
  COOP_ABORT_CHAIN = 1,         /* the one-launch BPTT chain gave up: a hand-off timed out, or somebody else gave up */
  COOP_ABORT_CHAIN_OFF_XCD = 2, /* ... a workgroup of it was not on the XCD its number implies (or drew a surplus seat) */
  COOP_ABORT_XCHG_BARRIER = 6,  /* a barrier of the kernel-issued exchange timed out (k_xchg_barrier) */
  COOP_ABORT_FWD_TOP = 7        /* the text step's forward + top launch gave up */
};

enum { COOP_XCDS = 8, COOP_SEATS = 32, COOP_WGS = COOP_XCDS * COOP_SEATS, COOP_CU_KEYS = 256 };
#define COOP_NO_SEAT 0xffffffffu /* every byte 0xff: no such CU */

/* what k_residency_probe leaves: how many of its 256 workgroups arrived, whether one of them timed out waiting for the
 * others, and per workgroup the XCD (HW_REG_XCC_ID) and the CU's hardware number (HW_REG_HW_ID's se / sh / cu bits) */
typedef struct CoopProbe {
  unsigned arrived, fail;
  unsigned xcc[COOP_WGS];
  unsigned cu_key[COOP_WGS];
} CoopProbe;

/* The seat of the CU a workgroup finds itself on, by XCD and the CU's hardware number: made once from the probe,
 * COOP_NO_SEAT: no such CU.  In device memory, never written while a launch runs (how the kernels read it: k_coop.h). */
typedef struct SeatTable {
  unsigned seat[COOP_XCDS][COOP_CU_KEYS];
} SeatTable;

/* what the probe found and what the process has said since, for a launch that is about to seat its workgroups */
typedef struct SeatRule {
  int resident; /* 256 workgroups were resident together, one per CU, and no launch has given up since */
  int table;    /* the seat table is there */
  int tickets;  /* side stream, RCCL group (ramd_note_side_stream): the chain draws tickets */
  int mode;     /* coop_seat_mode: how a chain launch seats its workgroups */
  const unsigned *seats; /* SeatTable, device */
} SeatRule;

/* all 256 workgroups were on the device together, one per CU */
static inline int coop_resident(const CoopProbe *p) { return !p->fail && p->arrived == (unsigned)COOP_WGS; }

/* the dispatcher dealt the workgroups to the XCDs in turn: workgroup i on XCD i % 8 */
static inline int coop_in_turn(const CoopProbe *p) {
  for (int i = 0; i < COOP_WGS; i++)
    if (p->xcc[i] != (unsigned)(i % COOP_XCDS)) return 0;
  return 1;
}

/* The 256 workgroups of the probe, one per CU, named 32 different CUs on each XCD: their hardware numbers (the low 8
 * bits of the key) in ascending order are seats 0 .. 31.  0: an XCD has other than 32 workgroups, or two of them one CU
 * number -- not what the launches rely on, no table. */
static inline int coop_seat_table(const CoopProbe *p, SeatTable *t) {
  memset(t, 0xff, sizeof(*t));
  for (int x = 0; x < COOP_XCDS; x++) {
    unsigned char named[COOP_CU_KEYS] = {0};
    unsigned n = 0, seat = 0;
    for (int i = 0; i < COOP_WGS; i++) {
      if (p->xcc[i] != (unsigned)x) continue;
      n++;
      if (named[p->cu_key[i] & 0xffu]++) return 0; /* two workgroups on one CU number */
    }
    if (n != (unsigned)COOP_SEATS) return 0;
    for (int k = 0; k < COOP_CU_KEYS; k++)
      if (named[k]) t->seat[x][k] = seat++;
  }
  return 1;
}

/* How a chain launch seats its workgroups.  2: from the CU's hardware number through the table (the default: robust
 * beside other work); 1: from the workgroup NUMBER, only on request (RECUR_AMD_XCD_STATIC=1), where the probe found
 * the workgroups dealt in turn, and not beside this process's own side streams -- anything else that runs on the GPU
 * beside the chain makes the dispatcher interleave the launches, and a chain whose workgroup is not where its number
 * says gives the launch up (COOP_ABORT_CHAIN_OFF_XCD); 0: a ticket per workgroup.
 * `table`: coop_seat_table made one and RECUR_AMD_XCD_TABLE (default 1) is not 0; `static_requested`:
 * RECUR_AMD_XCD_STATIC (default 0). */
static inline int coop_seat_mode(int table, int static_requested, int in_turn, int side_streams) {
  return table ? 2 : (static_requested && in_turn && !side_streams) ? 1 : 0;
}

/* Flags are launch numbers that only grow and compare as unsigned numbers; the launcher clears the flags and starts the
 * sequence over long before they wrap.  The chain's flags are seq * COOP_CHAIN_EPOCH + step (depth <= 60), the forward +
 * top launch's are seq itself.  The launcher asks before it counts up, so the largest seq in use IS the limit. */
#define COOP_CHAIN_EPOCH 64u
#define COOP_CHAIN_SEQ_LIMIT (1u << 25)
#define COOP_FWD_TOP_SEQ_LIMIT (1u << 30)
static inline int coop_seq_starts_over(unsigned seq, unsigned limit) { return seq >= limit; }
static_assert((unsigned long long)COOP_CHAIN_SEQ_LIMIT * COOP_CHAIN_EPOCH + (COOP_CHAIN_EPOCH - 1u) < (1ull << 32) &&
                  (unsigned long long)COOP_FWD_TOP_SEQ_LIMIT < (1ull << 32),
              "the largest flag a launch can write fits 32 bits");
