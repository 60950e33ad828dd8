/* seqs_plan.h -- how the frames of a batch of dense feature sequences are staged for rnn_amd_run_sequences (seqs_api.c):
 * the segments, their live rows and the offsets into the staging buffers, apart from the copies and the launches.
 *
 * The order and the waves are texts_plan.h's: a sequence of n frames is a text of n + 1 symbols (n forward passes), so a
 * sequence without a frame takes no row, the rows go longest first in waves of W, and the rows that still run at frame t
 * are a prefix of their wave.  What is new is that a frame costs 4 * input_size bytes where a symbol costs one: a wave's
 * frames are not uploaded whole.  A wave runs in SEGMENTS of at most F frames, segment q being the wave's frames
 * [q * F, min((q + 1) * F, steps)).  In a segment
 *   live      = texts_plan_active(wave, q * F): the rows that have a frame in it, a prefix of the wave;
 *   count[j]  = min(n_j - q * F, F) for a live row j, its frames in the segment (at least 1), 0 for the others;
 *   off[j]    = count[0] + ... + count[j - 1]: where row j's frames start in the segment's staging buffers, IN FRAMES.
 * The three staging buffers of a segment share that one offset, each times its own entries per frame: row j's frame
 * q * F + i is staged at (off[j] + i) * input_size floats of the inputs, its answers come back at (off[j] + i) *
 * output_size floats, its winners at (off[j] + i) * n_groups bytes.  Every (row, frame) has exactly one slot, in exactly
 * one segment.  The buffers are sized by the largest segment -- the first of the first wave: lengths descend through the
 * plan -- and not by the longest sequence.  The rows' states stay in their state rows between segments.
 *
 * F <= 0 asks for the default, seqs_plan_default_segment(): the largest F whose input staging for a full wave,
 * W * F * input_size * 4 bytes, stays within SEQS_STAGE_BYTES, and at least 1: 64 frames at 32 features.  (Measured with
 * tools/gpu_seqs_rate.py, profiles/r07_seqs_rate.txt: 256 recordings of 400 - 600 frames run as fast or faster in segments
 * of 64 frames than in segments of 512 -- a 16 MiB budget, the first choice -- and slower in segments of 8.)
 *
 * No HIP: the host compiler alone builds it and tests/test_seqs_plan.py asks it on a machine without a GPU.  Plain C (and
 * valid C++). */
#ifndef RAMD_SEQS_PLAN_H
#define RAMD_SEQS_PLAN_H 1
#include "texts_plan.h"

#define SEQS_STAGE_BYTES (2u << 20) /* a full wave's input staging per segment, at the default segment */

/* the segment length in frames for segment_frames as the caller gave it (<= 0: the default) */
static inline int seqs_plan_default_segment(int input_size, int width) {
  if (width < 1) {
    width = TEXTS_PLAN_WIDTH;
  }
  const unsigned long long per_frame = (unsigned long long)width * (unsigned long long)(input_size > 0 ? input_size : 1) * 4u;
  const unsigned long long f = SEQS_STAGE_BYTES / per_frame;
  return f < 1 ? 1 : f > 0x7fffffffu ? 0x7fffffff : (int)f;
}
static inline int seqs_plan_segment_frames(int segment_frames, int input_size, int width) {
  return segment_frames > 0 ? segment_frames : seqs_plan_default_segment(input_size, width);
}

/* the plan of n_seqs sequences of n_frames[k] frames: texts_plan_make on lens[k] = n_frames[k] + 1 (p->len[r] - 1 is row
 * r's frame count).  lens[n_seqs] is the caller's and is left filled: the states' rule for the sequences without a row
 * (texts_states.h) reads the same lengths.  Every n_frames[k] is >= 0 and < INT_MAX (the caller has checked).  Returns 0,
 * or -1 out of memory. */
static inline int seqs_plan_make(TextsPlan *p, const int *n_frames, int n_seqs, int width, int *lens) {
  for (int k = 0; k < n_seqs; k++) {
    lens[k] = n_frames[k] + 1;
  }
  return texts_plan_make(p, lens, NULL, n_seqs, width);
}

/* the segments of wave w: its steps in pieces of F frames */
static inline int seqs_plan_segments(const TextsPlan *p, int w, int F) {
  return (int)(((long long)p->waves[w].steps + F - 1) / F);
}

/* segment q of wave w: *t0 its first frame, *frames how many frames of the wave it covers, *live its rows; count[j] and
 * off[j] for ALL the wave's nrows rows (count 0 and off = the total behind the live ones).  Returns the segment's total
 * frames over its rows: the staging buffers' extent, times the entries per frame. */
static inline unsigned long long seqs_plan_segment(const TextsPlan *p, int w, int q, int F, int *t0, int *frames, int *live,
                                                   int *count, unsigned long long *off) {
  const TextsWave *wave = &p->waves[w];
  const int *len = p->len + wave->row0;
  const long long first = (long long)q * F;
  const long long left = (long long)wave->steps - first;
  *t0 = (int)first;
  *frames = (int)(left < F ? left : F);
  *live = texts_plan_active(p, w, (int)first);
  unsigned long long at = 0;
  for (int j = 0; j < wave->nrows; j++) {
    const long long mine = (long long)(len[j] - 1) - first; /* row j's frames from the segment's first on */
    count[j] = mine <= 0 ? 0 : (int)(mine < F ? mine : F);
    off[j] = at;
    at += (unsigned long long)count[j];
  }
  return at;
}

/* the largest segment total of the plan, in frames: wave 0's first segment */
static inline unsigned long long seqs_plan_largest(const TextsPlan *p, int F) {
  unsigned long long at = 0;
  if (p->n_waves < 1) {
    return 0;
  }
  for (int j = 0; j < p->waves[0].nrows; j++) {
    const int n = p->len[j] - 1;
    at += (unsigned long long)(n < F ? n : F);
  }
  return at;
}

#endif
