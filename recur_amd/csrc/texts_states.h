/* texts_states.h -- how the per-text hidden states of the batched text calls (rnn_amd_run_texts_from, _trace_texts_from,
 * _continue_texts_from) travel between the caller's arrays and a wave's state rows: the permutation, apart from the copies
 * to and from the device.
 *
 * A state is a row of `width` floats laid out as RecurNN.hidden_layer is (width = h_size), of which only the elements
 * [1, hidden] carry information: assemble_input_row (k_common.h) reads no other.  The caller's arrays are
 * [n_texts][width] in the caller's order; a wave's staging buffer is [nrows][width] in plan order (texts_plan.h: longest
 * first, waves of W rows), row j of wave w being the caller's text order[row0 + j].  Three rules, each stated once:
 *   pack    the wave's start states into the staging buffer: from h_in, or -- h_in NULL -- every row from one fallback
 *           row (the net's hidden row).  Only [1, hidden] is read; element 0 and the padding are written as zeros.
 *   unpack  the wave's final states from the staging buffer to h_out, whole rows.
 *   fill    the texts that take no row (shorter than 2 symbols): their final state is their start state.
 * h_out may be h_in (an update in place): a wave's pack is complete before its unpack begins, waves do not share texts,
 * and the fill of a text in place writes what is there.  No HIP: the host compiler alone builds it and
 * tests/test_texts_states.py asks it on a machine without a GPU.  Plain C (and valid C++). */
#ifndef RAMD_TEXTS_STATES_H
#define RAMD_TEXTS_STATES_H 1
#include <string.h>
#include "texts_plan.h"

/* one start state into dst: src's elements [1, hidden], zeros around them */
static inline void texts_state_take(float *dst, const float *src, int width, int hidden) {
  dst[0] = 0.0f;
  memmove(dst + 1, src + 1, (size_t)hidden * sizeof(float));
  for (int i = hidden + 1; i < width; i++) {
    dst[i] = 0.0f;
  }
}

/* staging[j] = the start state of wave w's row j, for its nrows rows */
static inline void texts_states_pack(const TextsPlan *p, int w, const float *h_in, const float *fallback, int width,
                                     int hidden, float *staging) {
  const TextsWave *wave = &p->waves[w];
  for (int j = 0; j < wave->nrows; j++) {
    const float *src = h_in ? h_in + (size_t)p->order[wave->row0 + j] * width : fallback;
    texts_state_take(staging + (size_t)j * width, src, width, hidden);
  }
}

/* h_out[order[row0 + j]] = staging[j], for wave w's nrows rows */
static inline void texts_states_unpack(const TextsPlan *p, int w, const float *staging, int width, float *h_out) {
  const TextsWave *wave = &p->waves[w];
  for (int j = 0; j < wave->nrows; j++) {
    memcpy(h_out + (size_t)p->order[wave->row0 + j] * width, staging + (size_t)j * width, (size_t)width * sizeof(float));
  }
}

/* the texts without a row (lens[k] < 2, as texts_plan_make counts them): h_out[k] = their start state */
static inline void texts_states_fill_rowless(const int *lens, int n_texts, const float *h_in, const float *fallback,
                                             int width, int hidden, float *h_out) {
  for (int k = 0; k < n_texts; k++) {
    if (lens[k] < 2) {
      texts_state_take(h_out + (size_t)k * width, h_in ? h_in + (size_t)k * width : fallback, width, hidden);
    }
  }
}

#endif
