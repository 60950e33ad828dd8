/* automaton_rule.h -- how rnnca's automaton makes the next frame from the last one, stated once: for k_automaton_step
 * (kernels_rows.hip), which runs it with one workgroup per cell, for automaton_api.c (gnu11 C: the refusals, the offset
 * pattern) and for any host compiler alone (tests/automaton_rule_harness.cpp runs it under g++ against numpy and the
 * oracle).  No HIP header is needed: under hipcc the functions are host and device functions, elsewhere plain inline
 * ones.  The level rule takes the exponential as an argument, as sample_rule.h's softmax does, and is C++; the rest is C.
 *
 * The arithmetic is the reference's, operation for operation, because a frame is bytes: one input that rounds the other
 * way can move a level, and that level is every neighbour's input in the next frame.
 *   source cell      (gstrnnca.c:644-667) the pixel that offset (dx, dy) names at cell (cx, cy): edges != 0 clamps x and
 *                    y to the grid; edges == 0 wraps ONCE -- one width or height is added or taken off, so an offset as
 *                    long as the grid leaves the plane (automaton_wrap_reaches: the call refuses it); y * width + x
 *   inputs of a cell (gstrnnca.c:669-691) len_y luma values, then len_c pairs (Cb, Cr), then the position.  A byte b is
 *                    b * (1.0f / 255.0f): a multiplication by the rounded reciprocal, not a division.  The position is
 *                    xx = cx * 1.0f / width, yy = cy * 1.0f / height, and with len_pos == 3 a third input
 *                    0.5 - ((yy - 0.5) * (yy - 0.5) + (xx - 0.5) * (xx - 0.5)), which C evaluates in double and rounds
 *                    to float once
 *   level            (gstrnnca.c:816, 825; badmaths.h:15-44) a = 1.0f / (1.0f + fast_expf(-out)); the byte is the
 *                    truncation of a * 255.9f.  What C leaves undefined is defined here: a scaled value outside [0, 256)
 *                    stores 0 if it is NaN or negative and 255 otherwise; an output that is not finite does not enter
 *                    the exponential (whose range reduction would not end on it) and takes the exponential's limit
 *   offset pattern   (host only; setup_inputs, gstrnnca.c:375-439) a string such as "Y00120111C0111" into the Y and the C
 *                    list of (dx, dy) pairs: a digit pair is (min, max), unfolded over its sign symmetries and the
 *                    diagonal swap in the reference's order; any other character is skipped
 * A GCC caller of the input rule compiles with -ffp-contract=off (clang takes the pragma below). */
#ifndef RAMD_AUTOMATON_RULE_H
#define RAMD_AUTOMATON_RULE_H 1

#ifndef RAMD_HD
#if defined(__HIP__) || defined(__HIPCC__)
#define RAMD_HD __attribute__((host)) __attribute__((device)) inline
#elif defined(__cplusplus)
#define RAMD_HD inline
#else
#define RAMD_HD static inline
#endif
#endif
#ifndef RAMD_FP_UNFUSED
#if defined(__clang__)
#define RAMD_FP_UNFUSED _Pragma("clang fp contract(off)")
#else
#define RAMD_FP_UNFUSED
#endif
#endif

#define AUTOMATON_DEFAULT_PATTERN "Y00120111C0111"

/* the grid and what a cell sees of it (RnnAmdAutomaton's fields; the offset lists wherever the reader can reach them) */
typedef struct AutomatonRule {
  int width, height;
  const int *offsets_y; /* [len_y] (dx, dy) */
  int len_y;
  const int *offsets_c; /* [len_c] (dx, dy) */
  int len_c;
  int len_pos; /* 2 or 3 */
  int edges;   /* non-zero: clamp; 0: wrap once */
} AutomatonRule;

/* The one launch between two forward passes of rnn_amd_run_automaton (k_automaton_step, kernels_rows.hip; the launcher is
 * declared in ramd_internal.h), for the width * height cells of g on forward-only state rows, cell c on row row0 + c; g's
 * offset lists are device arrays, and with edges == 0 the caller has refused offsets the single wrap does not bring back.
 * Two halves:
 *   paint (paint != NULL; not in a call's first launch): the three levels of every cell's outputs, which the forward pass
 *     just left in its out row, as bytes into the planes of the frame paint[3][cells].  Every byte has one writer.
 *   feed (feed != 0; not in a call's last launch): the input row of every cell's next forward pass, from the levels of its
 *     neighbours -- gathered from the bytes of seed[3][cells] (a call's first launch), or with a NULL seed made from the
 *     neighbours' out rows, which is the frame this launch paints -- and the position, on the row's hidden values, or on
 *     hid0's when that is not NULL.
 * All pointers are device pointers. */
typedef struct RamdAutomatonStep {
  AutomatonRule g;           /* the grid                                                 */
  const unsigned char *seed; /* [3][cells] the frame the first feed gathers from, or NULL */
  unsigned char *paint;      /* [3][cells] the frame to paint, or NULL                    */
  const float *hid0;         /* the hidden row of the first feed, or NULL                 */
  int row0;                  /* state row of cell 0 (forward-only)                        */
  int feed;
} RamdAutomatonStep;

RAMD_HD int automaton_input_size(const AutomatonRule *g) { return g->len_y + 2 * g->len_c + g->len_pos; }

/* gstrnnca.c:644-667 */
RAMD_HD int automaton_source_cell(int dx, int dy, int cx, int cy, int width, int height, int edges) {
  int x = cx + dx;
  int y = cy + dy;
  if (edges) {
    y = y > height - 1 ? height - 1 : y;
    y = y < 0 ? 0 : y;
    x = x > width - 1 ? width - 1 : x;
    x = x < 0 ? 0 : x;
  } else {
    if (y < 0) {
      y += height;
    } else if (y >= height) {
      y -= height;
    }
    if (x < 0) {
      x += width;
    } else if (x >= width) {
      x -= width;
    }
  }
  return y * width + x;
}

/* whether the single wrap brings offset (dx, dy) back into the plane from every cell */
RAMD_HD int automaton_wrap_reaches(int dx, int dy, int width, int height) {
  return dx > -width && dx < width && dy > -height && dy < height;
}

/* BYTE_TO_UNIT (gstrnnca.c:640) */
RAMD_HD float automaton_unit(unsigned char b) {
  RAMD_FP_UNFUSED
  return b * (1.0f / 255.0f);
}

/* the position inputs (gstrnnca.c:684-690): which = 0: xx, 1: yy, 2: the third */
RAMD_HD float automaton_position(int which, int cx, int cy, int width, int height) {
  RAMD_FP_UNFUSED
  const float xx = cx * 1.0f / width;
  const float yy = cy * 1.0f / height;
  if (which == 0) {
    return xx;
  }
  if (which == 1) {
    return yy;
  }
  const double ys = ((double)yy - 0.5) * ((double)yy - 0.5);
  const double xs = ((double)xx - 0.5) * ((double)xx - 0.5);
  const double both = ys + xs;
  return (float)(0.5 - both);
}

/* UNIT_TO_BYTE and the store into a byte (gstrnnca.c:642, 825) */
RAMD_HD unsigned char automaton_byte(float scaled) {
  if (scaled >= 0.0f && scaled < 256.0f) {
    return (unsigned char)(int)scaled;
  }
  return scaled > 0.0f ? 255 : 0; /* NaN and the negative ones: 0 */
}

/* which plane's byte of which cell input i of cell (cx, cy) is made from: returns the plane (0 Y, 1 Cb, 2 Cr) and the
 * source cell in *cell, or -1 for a position input, with its number in *cell */
RAMD_HD int automaton_input_source(const AutomatonRule *g, int cx, int cy, int i, int *cell) {
  if (i < g->len_y) {
    *cell = automaton_source_cell(g->offsets_y[2 * i], g->offsets_y[2 * i + 1], cx, cy, g->width, g->height, g->edges);
    return 0;
  }
  i -= g->len_y;
  if (i < 2 * g->len_c) {
    const int *o = g->offsets_c + 2 * (i >> 1);
    *cell = automaton_source_cell(o[0], o[1], cx, cy, g->width, g->height, g->edges);
    return 1 + (i & 1);
  }
  *cell = i - 2 * g->len_c;
  return -1;
}

/* setup_inputs (gstrnnca.c:375-439): the pattern's Y and C offsets into the caller's arrays of max_pairs (dx, dy) pairs
 * each.  Returns 0, or -1 -- with nothing written behind either array -- when a list does not fit or an argument is NULL;
 * the lengths then say how far it got. */
RAMD_HD int automaton_parse_offsets(const char *pattern, int *offsets_y, int *len_y, int *offsets_c, int *len_c,
                                    int max_pairs) {
  if (!pattern || !offsets_y || !len_y || !offsets_c || !len_c) {
    return -1;
  }
  int *target = offsets_y;
  int *len = len_y;
  int pair[2] = {0, 0};
  int parity = 0;
  *len_y = 0;
  *len_c = 0;
  for (int i = 0; pattern[i]; i++) {
    const char c = pattern[i];
    if (c == 'Y') {
      len = len_y;
      target = offsets_y;
      continue;
    }
    if (c == 'C') {
      len = len_c;
      target = offsets_c;
      continue;
    }
    if (c < '0' || c > '9') {
      continue; /* (the reference warns and goes on) */
    }
    pair[parity] = c - '0';
    parity = 1 - parity;
    if (parity != 0) {
      continue;
    }
    int x = pair[0] < pair[1] ? pair[0] : pair[1];
    int y = pair[0] < pair[1] ? pair[1] : pair[0];
    /* the three symmetries (diagonal, horizontal, vertical) are variously cancelled out by zeros and x == y */
    do {
      do {
        do {
          if (*len >= max_pairs) {
            return -1;
          }
          target[*len * 2] = x;
          target[*len * 2 + 1] = y;
          *len += 1;
          y = -y;
        } while (y < 0);
        x = -x;
      } while (x < 0);
      const int swap = x;
      x = y;
      y = swap;
    } while (y < x);
  }
  return 0;
}

#ifdef __cplusplus
/* input i of cell (cx, cy); level(plane, cell) is the byte of the frame before: from memory, or made from a neighbour's
 * outputs by automaton_level */
template <class LEVEL>
RAMD_HD float automaton_input(const AutomatonRule &g, int cx, int cy, int i, const LEVEL &level) {
  int cell;
  const int plane = automaton_input_source(&g, cx, cy, i, &cell);
  return plane < 0 ? automaton_position(cell, cx, cy, g.width, g.height) : automaton_unit(level(plane, cell));
}

/* the level of one output: fast_sigmoid (badmaths.h:31-44) with the caller's fast exponential, then the byte */
template <class EXP>
RAMD_HD unsigned char automaton_level(float out, EXP fast_exp) {
  RAMD_FP_UNFUSED
  const float x = -out * 1.0f;
  float e;
  if (__builtin_fabsf(x) <= 3.0e38f) {
    e = fast_exp(x);
  } else if (x != x) {
    e = x;
  } else {
    e = x > 0.0f ? __builtin_inff() : 0.0f;
  }
  const float a = 1.0f / (1.0f + e);
  return automaton_byte(a * 255.9f);
}
#endif

#endif
