/* noise_ahead.h -- whether a forward pass may take the presynaptic noise that was generated ahead of it, stated once: for
 * the host code that generates it (noise_ahead.c) and for any host compiler alone (tests/noise_ahead_harness.cpp asks it
 * under g++, tests/test_noise_ahead.py holds the answers to a model of the generators' history).  No HIP header, no
 * device pointer, no event.  Plain C and valid C++.
 *
 * A stream's generator is a sequential recurrence, so a pass's noise is generated on a second stream while the main
 * stream does something else, into one of two slots: the values and the generator states after them.  The pass adopts
 * them only if the generators stand exactly where the slot's values started.  Nothing reads the generators back to see:
 * every event that moves them is counted (`moves`), and a slot is stamped with the count that must stand when its pass
 * begins.
 *   slot `head` is the one the NEXT pass takes; a slot filled one pass further ahead is the other one.
 *   A slot filled from the generators themselves is stamped with the current count.
 *   A slot filled between a pass and the multi-head loss behind it starts from the states the pass adopted, past the
 *   loss's draws, which it makes itself from the classes on the device: the current count + 1.
 *   A slot filled two ahead starts from the states slot `head` leaves, past the draws of a loss whose classes nobody has
 *   yet: one draw per head but the stream's own, on the ASSUMPTION that every stream's own class is one of
 *   `assumed_classes` heads.  Its count is PREDICTED, head's + 2 (one pass, one loss): when that loss comes,
 *   noise_ahead_loss holds the assumption to the classes uploaded by then, and noise_ahead_host_write drops everything,
 *   because a different sequence of the same length -- an upload where the loss was expected -- would carry the same
 *   count.
 * Rows are state rows: a speculation is made for training sets only, whose state rows are their stream rows. */
#ifndef RAMD_NOISE_AHEAD_H
#define RAMD_NOISE_AHEAD_H 1

typedef struct NoiseAheadSlot {
  int pending;         /* filled, or being filled, and not yet taken or dropped */
  unsigned long version; /* `moves` as it must stand when the slot's pass begins */
  int row0, n;         /* the pass's rows */
  float level;         /* ... and its presynaptic_noise */
  int assumed_classes; /* != 0: generated past a loss of that many heads before its classes were known */
} NoiseAheadSlot;

typedef struct NoiseAhead {
  unsigned long moves;  /* events that moved a generator of the engine's */
  NoiseAheadSlot slot[2];
  int head;             /* the slot the next pass takes */
  int adopted;          /* the slot the last pass took its noise and states from, or -1 */
  int classes_in_range; /* every stream's class of the last multi-head upload is one of the heads */
} NoiseAhead;

/* where a launch starts from: the generators themselves, or the states slot 0 / 1 holds */
#define NOISE_AHEAD_GENERATORS (-1)

typedef struct NoiseAheadLaunch {
  int dst;       /* the slot filled */
  int src;       /* NOISE_AHEAD_GENERATORS, or the slot whose states the generator starts from */
  int n_classes; /* > 0: first the draws of a loss of that many heads, each stream's class read from the device */
  int skip;      /* ... or that many draws per stream */
  unsigned long version; /* what dst was stamped with */
  int assumed_classes;
} NoiseAheadLaunch;

/* an offer's answer: launches on the side stream, in this order.  behind_main: they are ordered behind the main stream's
 * work so far, ONE hand-over for all of them (the draws made so far, and the last reader of a slot that is filled again:
 * the pass that adopted it) -- set whenever there is a launch */
typedef struct NoiseAheadPlan {
  int n_launches, behind_main;
  NoiseAheadLaunch launch[2];
} NoiseAheadPlan;

static inline void noise_ahead_drop(NoiseAhead *a) { a->slot[0].pending = a->slot[1].pending = 0; }

static inline void noise_ahead_reset(NoiseAhead *a) {
  const NoiseAhead none = {0, {{0, 0, 0, 0, 0.0f, 0}, {0, 0, 0, 0, 0.0f, 0}}, 0, -1, 0};
  *a = none;
}

/* a generator was written from the host (a caller's draw, a per-net call's upload): nothing generated ahead from the
 * device's states can be right any more */
static inline void noise_ahead_host_write(NoiseAhead *a) {
  a->moves++;
  noise_ahead_drop(a);
}

/* the device image is freed, the slots' buffers with it */
static inline void noise_ahead_freed(NoiseAhead *a) {
  noise_ahead_drop(a);
  a->adopted = -1;
}

/* A forward pass of state rows [r0, r0 + n) at noise `level`; bottom: the net has a bottom layer.  Returns the slot the
 * pass takes its noise and states from, or -1: it runs the generators itself (or, level 0, draws nothing: no move then,
 * and what is pending stays).  What does not fit is dropped, both slots: the second hangs on the first. */
static inline int noise_ahead_pass(NoiseAhead *a, int r0, int n, float level, int bottom) {
  a->adopted = -1;
  if (level == 0.0f) {
    return -1;
  }
  const int k = a->head;
  const NoiseAheadSlot *s = &a->slot[k];
  if (s->pending && s->version == a->moves && s->row0 == r0 && s->n == n && s->level == level && !bottom) {
    a->slot[k].pending = 0;
    a->head = k ^ 1; /* (the other slot: the pass after this one, if it has been started) */
    a->adopted = k;
  } else {
    noise_ahead_drop(a);
  }
  a->moves++; /* the pass moves the generators, either way */
  return a->adopted;
}

static inline void noise_ahead_stamp_(NoiseAhead *a, NoiseAheadPlan *p, int dst, int src, int n_classes, int skip,
                                      unsigned long version, int assumed_classes, int row0, int n, float level) {
  const NoiseAheadSlot s = {1, version, row0, n, level, assumed_classes};
  const NoiseAheadLaunch l = {dst, src, n_classes, skip, version, assumed_classes};
  a->slot[dst] = s;
  p->launch[p->n_launches++] = l;
  p->behind_main = 1;
}

/* An offer to generate ahead for the next pass of rows [row0, row0 + n) at `level`.  loss_classes == 0: the last draw
 * before that pass has been made.  loss_classes > 0: between a pass and the multi-head loss of that many heads behind it,
 * where only the states the pass adopted are safe to start from.  mode: RECUR_AMD_NOISE_AHEAD's, 0 off, 1 one pass ahead,
 * otherwise two. */
static inline NoiseAheadPlan noise_ahead_offer(NoiseAhead *a, int row0, int n, float level, int loss_classes, int mode) {
  NoiseAheadPlan p = {0, 0, {{0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}}};
  if (mode == 0 || level == 0.0f || (loss_classes > 0 && a->adopted < 0)) {
    return p;
  }
  /* the next pass (slot head), unless an earlier offer has started it already */
  const int k = a->head, k2 = k ^ 1;
  if (!a->slot[k].pending) {
    if (loss_classes > 0) { /* (the loss that follows counts as one move) */
      noise_ahead_stamp_(a, &p, k, a->adopted, loss_classes, 0, a->moves + 1, 0, row0, n, level);
    } else {
      noise_ahead_stamp_(a, &p, k, NOISE_AHEAD_GENERATORS, 0, 0, a->moves, 0, row0, n, level);
    }
  }
  /* ... and, in the multi-head step, the pass after it: the generator then runs a whole generation ahead and is off the
   * critical path even where it is as long as the generation (32 streams per GPU) */
  const NoiseAheadSlot *h = &a->slot[k];
  if (mode != 1 && loss_classes > 0 && h->pending && !a->slot[k2].pending && h->row0 == row0 && h->n == n &&
      h->level == level) {
    noise_ahead_stamp_(a, &p, k2, k, 0, loss_classes - 1, h->version + 2, loss_classes, row0, n, level);
  }
  return p;
}

/* the classes of n streams were uploaded for a loss of n_classes heads */
static inline void noise_ahead_classes(NoiseAhead *a, const int *classes, int n, int n_classes) {
  int ok = 1;
  for (int j = 0; j < n; j++) {
    ok &= classes[j] >= 0 && classes[j] < n_classes;
  }
  a->classes_in_range = ok;
}

/* The multi-head loss of n_classes heads ran: its leak decisions are draws from the streams' generators.  Noise that was
 * generated past THIS loss before its classes were known is dropped unless the assumption held -- and the other slot with
 * it: it hangs on that one, or is the pass in between, which is redone.  Returns whether anything was dropped. */
static inline int noise_ahead_loss(NoiseAhead *a, int n_classes) {
  int dropped = 0;
  a->moves++;
  for (int k = 0; k < 2; k++) {
    const NoiseAheadSlot *s = &a->slot[k];
    if (s->pending && s->assumed_classes && s->version == a->moves &&
        (s->assumed_classes != n_classes || !a->classes_in_range)) {
      dropped = 1;
    }
  }
  if (dropped) {
    noise_ahead_drop(a);
  }
  return dropped;
}

#endif
