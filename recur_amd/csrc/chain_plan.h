// chain_plan.h -- which launches the BPTT chain (ramd_chain_steps) gets: the rule, apart from the launches.
//
// ramd_plan_chain() reads the shape, the call's rows, of RamdBuffers only uniform_idx, the RECUR_AMD_CHAIN_* switches and
// one fact about the process -- whether the one-launch chain is available (the residency probe has validated the device
// and no launch has given up: kernels_chain.hip) -- and fills a ChainPlan: the rows the one-launch chain runs over, and
// the launch-per-step form that runs where it does not take the call or gives up.  chain_segment() cuts those rows into
// the launches of k_chain_persist.  It makes no HIP call and follows no device pointer, so the host compiler alone builds
// it and tests/test_chain_plan.py asks it on a machine without a GPU.  Every switch that decides which launches the
// chain gets is read here.
#pragma once
#include "ramd_internal.h"
#include "k_tiles.h"

enum ChainForm {
  CHAIN_WIDE, /* k_chain_wide<NS, MT>: 64 x 64 or 32 x 64 tiles */
  CHAIN_MAIN  /* k_chain_main<UNI, NS>: 32 x 32 tiles */
};

/* the launch-per-step form: D launches of one kernel */
struct ChainSteps {
  ChainForm form;
  bool uniform;    /* CHAIN_MAIN: every stream at the same ring position */
  int ns, nstages; /* K stages (ns 0: any number of them, nstages at run time) */
  int mt;          /* streams per row tile: 64 or 32 (CHAIN_WIDE), 32 (CHAIN_MAIN) */
  int tm, tn, blocks;
  int tn_parts;    /* partial sums of squares per (step, stream) it leaves: one per column tile */
};

struct ChainPlan {
  int row0, nrows;
  int chain_rows; /* nrows, padded to whole 16-row tiles where Scap has room */
  bool windowed;  /* one launch over the tiles from the tile boundary below row0 */
  int span_base, span;
  int seg_rows;   /* the rows chain_segment() cuts into launches; 0: the one-launch chain does not take the call */
  int nt, seats;  /* column tiles of a row tile; row tiles per launch */
  bool one_ok;    /* RECUR_AMD_CHAIN_ONE */
  ChainSteps steps;
};

/* one launch of k_chain_persist<ACT, K, one, pad, .> over rows [row0, row0 + nrows), of which [vlo, nvalid) are the call's */
struct ChainSegment {
  int row0, nrows;
  bool one, pad; /* 16-stream row tiles; rows of the launch that are not the call's: multiplied along, never stored */
  int nvalid, vlo;
  int workers, idle_only; /* who shares a request for the top layer's delta (HoWork) */
  int early;              /* K blocks of each burst issued under the row stores' drain (k_chain_persist_early, PC_EARLY of k_tiles.h);
                           * 0: k_chain_persist.  The launcher has the last word: a launch that carries the tail for DENSE inputs
                           * (known at the launch, not here) keeps k_chain_persist<.., XD>, which has no early form */
};

/* row tiles per launch: 8 XCDs x (32 seats / column tiles) */
static inline int chain_persist_seats(const RamdShape *sh) {
  const int nt = sh->hidden_size / 32; /* column tiles; the one-launch chain exists for 8, 16 and 32 of them */
  return nt > 0 && nt <= 32 ? 8 * (32 / nt) : 0;
}
/* 16-stream row tiles (one sub-chain per workgroup) when they all still fit one launch: twice the
 * CUs for a small set; otherwise 32-stream tiles, which move more streams per microsecond */
static inline bool chain_persist_one(int seats, bool one_ok, int nrows) {
  return nrows / 16 <= seats && (nrows % 32 != 0 || one_ok);
}
static inline int chain_persist_rows(int seats, bool one) { return seats * (one ? 16 : 32); }

/* K blocks (8 MFMAs each) of every half-step's burst that the multiplying waves issue while the finish's row stores drain
 * (k_chain_persist.h, EARLY): hidden 1024 with 32-stream row tiles, where profiles/NOTES_r20.md measured it; 16-stream tiles
 * have no drain beside a burst, and hidden 512 / 256 stay as they were.  RECUR_AMD_CHAIN_EARLY=0: k_chain_persist as before. */
static inline int chain_early_blocks(int hidden_size, bool one, bool pad) {
  return hidden_size == 1024 && !one && !pad && env_int("RECUR_AMD_CHAIN_EARLY", 1) ? PC_EARLY : 0;
}

/* the one-launch chain takes `nrows` rows of this shape (whether it is available is the launcher's to know) */
static inline bool chain_persist_takes(const RamdShape *sh, const RamdBuffers *b, int nrows) {
  const int hs = sh->hidden_size;
  return b->uniform_idx >= 0 && (hs == 1024 || hs == 512 || hs == 256) && nrows >= 1 && nrows % 16 == 0 && sh->D <= 60 &&
         env_int("RECUR_AMD_CHAIN_PERSIST", 1);
}

/* a set that is not whole 16-row tiles runs over the rows above it (Scap is a multiple of 16:
 * they exist), which are multiplied along and never stored (pad) -- a one-net trainer or a
 * per-net call then takes the one-launch chain with a single tile instead of D launches */
static inline int chain_padded_rows(const RamdShape *sh, int row0, int nrows) {
  const int up = (nrows + 15) & ~15;
  return nrows % 16 != 0 && row0 + up <= sh->Scap ? up : nrows;
}
/* ... and a small set that does not start on a tile boundary (a per-net call on stream j):
 * the tiles from the boundary below it, one launch -- where those rows exist */
static inline bool chain_window(const RamdShape *sh, int row0, int nrows, int *base, int *span) {
  *base = row0 & ~15;
  *span = ((row0 + nrows + 15) & ~15) - *base;
  return *base != row0 && *base + *span <= sh->Scap;
}

/* The call's shape qualifies for the one-launch chain, as a window or as its own rows: the launcher then needs to know
 * whether the chain is available, which costs the probe once per process.  (A window of more row tiles than a launch has
 * seats asks too and then runs a launch per step unless its own rows qualify: the order the launcher always had.) */
static inline bool chain_persist_wanted(const RamdShape *sh, const RamdBuffers *b, int row0, int nrows) {
  int base, span;
  return (chain_window(sh, row0, nrows, &base, &span) && chain_persist_takes(sh, b, span)) ||
         chain_persist_takes(sh, b, chain_padded_rows(sh, row0, nrows));
}

static inline ChainSteps chain_plan_steps(const RamdShape *sh, const RamdBuffers *b, int nrows) {
  ChainSteps f = {};
  const int hs = sh->hidden_size;
  f.uniform = b->uniform_idx >= 0;
  /* big sets of a wide net: 64 x 64 tiles (k_chain_wide), one partial sum per 64 columns */
  const int wide_ns = hs / WK;
  /* ... as 32 x 64 tiles where that fills more of the chip: fewer than 192 tiles of 64 streams, and streams a multiple of 32 */
  const bool wide_half = f.uniform && nrows % 32 == 0 && hs % WN == 0 && (nrows / WM) * (hs / WN) < 192 &&
                         (nrows / 32) * (hs / WN) >= 128 && env_int("RECUR_AMD_CHAIN_WIDE_HALF", 1);
  const bool wide = f.uniform && (nrows % WM == 0 || wide_half) && hs % WN == 0 &&
                    (wide_ns == 16 || wide_ns == 24 || wide_ns == 32) && ((nrows / WM) * (hs / WN) >= 128 || wide_half) &&
                    env_int("RECUR_AMD_CHAIN_WIDE", 1);
  if (wide) {
    f.form = CHAIN_WIDE;
    f.ns = f.nstages = wide_ns;
    f.mt = wide_half ? 32 : WM;
    f.tm = nrows / f.mt;
    f.tn = hs / WN;
  } else {
    f.form = CHAIN_MAIN;
    f.nstages = (hs + CK - 1) / CK; /* K = the hidden columns 1..hidden_size */
    const bool unrolled = f.uniform && hs % CK == 0 && (f.nstages == 2 || f.nstages == 4 || f.nstages == 8 || f.nstages == 16);
    f.ns = unrolled ? f.nstages : 0;
    f.mt = CM;
    f.tm = (nrows + CM - 1) / CM;
    f.tn = (hs + CN - 1) / CN;
  }
  f.blocks = ((f.tn + 7) / 8) * 8 * f.tm;
  f.tn_parts = f.tn;
  return f;
}

static inline ChainPlan ramd_plan_chain(const RamdShape *sh, const RamdBuffers *b, int row0, int nrows, bool available) {
  ChainPlan p = {};
  p.row0 = row0, p.nrows = nrows;
  p.nt = sh->hidden_size / 32;
  p.seats = chain_persist_seats(sh);
  p.one_ok = env_int("RECUR_AMD_CHAIN_ONE", 1) != 0;
  p.chain_rows = chain_padded_rows(sh, row0, nrows);
  p.windowed = chain_window(sh, row0, nrows, &p.span_base, &p.span) && available && chain_persist_takes(sh, b, p.span) &&
               p.span / 16 <= p.seats;
  if (p.windowed)
    p.seg_rows = p.span;
  else if (available && chain_persist_takes(sh, b, p.chain_rows))
    p.seg_rows = p.chain_rows;
  p.steps = chain_plan_steps(sh, b, nrows);
  return p;
}

/* The launch of the one-launch chain that starts `r` rows into the plan's seg_rows (false: there is none; the next one
 * starts at r + nrows): as many row tiles per launch as there are seats, more streams: more launches. */
static inline bool chain_segment(const ChainPlan &p, int r, ChainSegment *s) {
  if (r >= p.seg_rows) return false;
  if (p.windowed) {
    *s = ChainSegment{p.span_base, p.span, true, true, p.row0 - p.span_base + p.nrows, p.row0 - p.span_base, 0, 0};
  } else {
    /* (an odd number of 16-stream tiles beyond one launch: 32-stream tiles, the last 16 streams alone) */
    const int left = p.chain_rows - r, real_left = p.nrows - r;
    bool one = chain_persist_one(p.seats, p.one_ok, left);
    int n = 0;
    if (!one) { /* 32-stream tiles over whole, real tiles only */
      n = real_left & ~31;
      if (n > chain_persist_rows(p.seats, false)) n = chain_persist_rows(p.seats, false);
      if (n == 0) one = true;
    }
    if (one) {
      n = chain_persist_rows(p.seats, true);
      if (n > left) n = left;
    }
    const int nvalid = real_left < n ? real_left : n;
    *s = ChainSegment{p.row0 + r, n, one, one && nvalid < n, nvalid, 0, 0, 0};
  }
  /* the launch's workgroups without chain work, if they are at least half of it, else all 256 */
  const int busy = (s->nrows / (s->one ? 16 : 32)) * p.nt;
  s->idle_only = 256 - busy >= 128;
  s->workers = s->idle_only ? 256 - busy : 256;
  s->early = chain_early_blocks(32 * p.nt, s->one, s->pad);
  return true;
}
