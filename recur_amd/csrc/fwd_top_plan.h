// fwd_top_plan.h -- whether a forward pass that stops for the text step's top launch (RAMD_FWD_FOR_TEXT_TOP) is taken,
// top layer included, by the ONE launch k_fwd_top (k_fwd_top.h) instead of k_fwd_fused + k_text_top2: the rule,
// apart from the launch.  Asked of the call's plan (ramd_plan_forward, whose answers stay what they are) before anything is
// launched; where this says no, that plan and ramd_launch_text_top run as before.  No HIP call and no device pointer followed: the host compiler alone builds it,
// and tests/test_fwd_top_plan.py asks it on a machine without a GPU.
//
// The launch is 256 workgroups of sixteen waves, one per CU; the 32 column-tile workgroups of a 32-stream row tile sit on
// ONE XCD (row tile g on XCD g, seats from the residency probe's table as the one-launch chain's: coop_rule.h, and DESIGN.md,
// "Launches whose workgroups wait for one another"), raise a flag each when
// their block of the new hidden sums is stored, and workgroup j of them then runs the top layer for stream j of the tile.
// So: hidden 1024 (32 column tiles = 32 seats = 32 streams), whole row tiles, at most eight of them, every stream at one
// ring position, text input, no presynaptic noise, no bottom layer, the shape k_text_top2 takes -- and the process not on
// tickets: with another queue's work beside the main one the 256 workgroups are not resident together for sure.
// And not in the chain's checked mode (RECUR_AMD_CHAIN_CHECK=1, RECUR_AMD_CHAIN_TEST_GIVEUP > 1): that mode is for a GPU
// where CUs may be missing, it reads the SHARED abort word behind every chain launch, clears it and redoes the chain --
// a give-up of this launch, first in the generation, would be taken for the chain's and its generation kept.
#pragma once
#include "fwd_plan.h"
#include "coop_rule.h" /* SeatRule: what the residency probe found, as plain numbers (kernels_coop.hip: coop_seat_rule) */

constexpr int FWD_TOP_HIDDEN = 1024, FWD_TOP_MAX_TILES = 8;

/* k_text_top2's preconditions (ramd_launch_text_top, kernels_loss.hip, asks this too): o_size a multiple of 4 up to 64
 * (sixteen lanes a row of W_ho), a wave's rows of W_ho in one batch of T2_NB x 4 */
static inline bool text_top2_takes(const RamdShape *sh) {
  return text_top_takes(sh) && sh->O % 4 == 0 && sh->O <= 64 && (sh->H + 15) / 16 <= 4 * T2_NB && env_int("RECUR_AMD_TEXT_TOP2", 1);
}
/* the one-launch chain's checked mode is on (kernels_chain.hip: launch_chain_persist) */
static inline bool chain_checked_mode(void) {
  return env_int("RECUR_AMD_CHAIN_CHECK", 0) || env_int("RECUR_AMD_CHAIN_TEST_GIVEUP", 0) > 1;
}

/* the static half: shape, call, switches and the call's plan p (asked first: the probe behind the other half costs a
 * launch, once).  The cheap refusals of the call come first: every forward pass of every shape asks. */
static inline bool fwd_top_shape_ok(const RamdShape *sh, const RamdBuffers *b, const RamdFwdCall *c, const FwdPlan &p) {
  if (c->want != RAMD_FWD_FOR_TEXT_TOP || c->mode != RAMD_IN_TEXT || !c->advance || c->rows_built || c->fwd_only || c->one_net)
    return false;
  if (!env_int("RECUR_AMD_FWD_TOP", 1) || chain_checked_mode()) return false;
  if (c->noise != 0.0f || sh->bI || sh->hidden_size != FWD_TOP_HIDDEN || !text_top2_takes(sh)) return false;
  if (b->uniform_idx < 0) return false; /* staggered rings */
  if (c->nrows <= 0 || c->nrows % CM != 0 || c->nrows > FWD_TOP_MAX_TILES * CM || c->row0 % CM != 0) return false;
  /* ... and the two launches would be k_fwd_fused<8> leaving its plane and partials: the same sums */
  return p.hidden == FH_FUSED && p.end == FE_LEFT && p.ht.ns == 8 && p.ht.tn == FWD_TOP_HIDDEN / CN && p.left.partials == p.ht.tn;
}

/* the other half: what the probe found */
static inline bool fwd_top_seats_ok(const SeatRule &seats) { return seats.resident && seats.table && !seats.tickets; }

static inline bool fwd_top_takes(const RamdShape *sh, const RamdBuffers *b, const RamdFwdCall *c, const FwdPlan &p,
                                 const SeatRule &seats) {
  return fwd_top_shape_ok(sh, b, c, p) && fwd_top_seats_ok(seats);
}
