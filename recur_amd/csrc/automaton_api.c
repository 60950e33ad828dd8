/* automaton_api.c -- rnnca's automaton played on the device, many frames in one run (gnu11 C): rnn_amd_run_automaton, the
 * batched form of fill_frame (gstrnnca.c:805-831: per cell fill_net_inputs from the frame before, rnn_opinion,
 * fast_sigmoid_array on three outputs, then the bytes of the next frame), and rnn_amd_automaton_parse_offsets
 * (setup_inputs, gstrnnca.c:375-439).  Every cell gets a forward-only state row of the engine's own, cell c the row
 * r0 + c, as seqs_api.c gives every sequence one; what differs from every other batched call is that the rows are not
 * independent -- frame t + 1 of a cell reads frame t of its neighbours -- so there are no waves: all width * height rows
 * run in lock step, and between two forward passes of them there is one launch (k_automaton_step, kernels_rows.hip) that
 * paints the frame just computed into the call's device frame buffer and builds every cell's next input row from its
 * neighbours' levels.  The rule itself is automaton_rule.h's.  The frames stay on the device and come back a segment at
 * a time: one copy, one synchronisation.  The states travel in one copy each way: all rows are live and lie in the
 * caller's order, so there is nothing to permute.  The net the caller passes is read -- its weights, its hidden row --
 * and not written; no generator is touched. */
#define RAMD_HIP_HOST 1
#include <limits.h>
#include "rnn_host.h"
#include "automaton_rule.h"
#include "texts_states.h"

#define WHO "rnn_amd_run_automaton"
/* the default segment: the largest count of frames whose bytes stay within this (at least one frame) */
#define AUTOMATON_SEGMENT_BYTES (16u << 20)

int rnn_amd_automaton_parse_offsets(const char *pattern, int *offsets_y, int *len_y, int *offsets_c, int *len_c,
                                    int max_pairs) {
  if (!pattern || !offsets_y || !len_y || !offsets_c || !len_c || max_pairs < 0) {
    fprintf(stderr, "librecur_amd: rnn_amd_automaton_parse_offsets: a NULL argument, or room for %d pairs\n", max_pairs);
    return -1;
  }
  if (automaton_parse_offsets(pattern, offsets_y, len_y, offsets_c, len_c, max_pairs)) {
    fprintf(stderr, "librecur_amd: rnn_amd_automaton_parse_offsets: '%s' has more than %d offsets in a list\n", pattern,
            max_pairs);
    return -1;
  }
  return 0;
}

/* the refusals, which need no device: -1 with a line on stderr, else 0 */
static int automaton_refused(const RecurNN *net, const RnnAmdAutomaton *ca, const u8 *seed, int n_frames, const u8 *frames) {
  if (!net || !ca || !seed || (n_frames > 0 && !frames)) {
    fprintf(stderr, "librecur_amd: " WHO ": a NULL net, geometry, seed or frame array\n");
    return -1;
  }
  if (n_frames < 0) {
    fprintf(stderr, "librecur_amd: " WHO ": %d frames\n", n_frames);
    return -1;
  }
  if (ca->width < 1 || ca->height < 1 || ca->width > INT_MAX / ca->height) {
    fprintf(stderr, "librecur_amd: " WHO ": a grid of %d x %d cells\n", ca->width, ca->height);
    return -1;
  }
  if (ca->len_y < 0 || ca->len_c < 0 || (ca->len_y > 0 && !ca->offsets_y) || (ca->len_c > 0 && !ca->offsets_c)) {
    fprintf(stderr, "librecur_amd: " WHO ": offset lists of %d and %d pairs, or a NULL one\n", ca->len_y, ca->len_c);
    return -1;
  }
  if (ca->len_pos != 2 && ca->len_pos != 3) {
    fprintf(stderr, "librecur_amd: " WHO ": %d position inputs (2 or 3)\n", ca->len_pos);
    return -1;
  }
  if ((long long)net->input_size != (long long)ca->len_y + 2LL * ca->len_c + ca->len_pos) {
    fprintf(stderr, "librecur_amd: " WHO ": the net has %d inputs, a cell %d + 2 * %d + %d\n", net->input_size, ca->len_y,
            ca->len_c, ca->len_pos);
    return -1;
  }
  if (net->output_size < 3) {
    fprintf(stderr, "librecur_amd: " WHO ": the net has %d outputs, a pixel three planes\n", net->output_size);
    return -1;
  }
  if (ramd_texts_net_refused(WHO, net, 0)) {
    return -1;
  }
  if (!ca->edges) {
    for (int k = 0; k < ca->len_y + ca->len_c; k++) {
      const int *o = k < ca->len_y ? ca->offsets_y + 2 * k : ca->offsets_c + 2 * (k - ca->len_y);
      if (!automaton_wrap_reaches(o[0], o[1], ca->width, ca->height)) {
        fprintf(stderr, "librecur_amd: " WHO ": offset (%d, %d) on a wrapped grid of %d x %d: the single wrap would leave "
                        "the plane\n", o[0], o[1], ca->width, ca->height);
        return -1;
      }
    }
  }
  return 0;
}

int rnn_amd_run_automaton(RecurNN *net, const RnnAmdAutomaton *ca, const u8 *seed, int n_frames, const float *h_in,
                          float *h_out, int segment_frames, u8 *frames) {
  if (automaton_refused(net, ca, seed, n_frames, frames)) {
    return -1;
  }
  const int cells = ca->width * ca->height;
  const size_t H = (size_t)net->h_size, frame_bytes = 3 * (size_t)cells;
  if (n_frames == 0) { /* nothing to play: every cell's final state is its start state, and no device is asked for */
    if (h_out) {
      float *row = NULL;
      if (!h_in) {
        row = ramd_zalloc(H * sizeof(float));
        ramd_texts_net_hidden_row(net, row);
      }
      for (int k = 0; k < cells; k++) {
        texts_state_take(h_out + k * H, h_in ? h_in + k * H : row, net->h_size, net->hidden_size);
      }
      free(row);
    }
    return 0;
  }
  size_t F = segment_frames > 0 ? (size_t)segment_frames : RAMD_MAX(AUTOMATON_SEGMENT_BYTES / frame_bytes, 1);
  F = RAMD_MIN(F, (size_t)n_frames);
  RamdRows rows;
  ramd_rows_open(&rows, net, cells);
  RamdEngine *e = rows.e;
  const RamdShape *s = &e->sh;
  /* every cell starts from the net's hidden row, or from its own state: all rows are live and lie in the caller's order */
  const float *hid0 = rows.hid0;
  if (h_in) {
    ramd_h2d(rows.states, h_in, (size_t)cells * s->H * sizeof(float));
    hid0 = NULL;
  }
  const size_t n_off = 2 * ((size_t)ca->len_y + (size_t)ca->len_c);
  int *d_off = ramd_rows_dev(&rows, (n_off ? n_off : 1) * sizeof(int));
  ramd_h2d(d_off, ca->offsets_y, 2 * (size_t)ca->len_y * sizeof(int));
  ramd_h2d(d_off + 2 * ca->len_y, ca->offsets_c, 2 * (size_t)ca->len_c * sizeof(int));
  u8 *d_seed = ramd_rows_dev(&rows, frame_bytes);
  u8 *d_frames = ramd_rows_dev(&rows, F * frame_bytes);
  ramd_h2d(d_seed, seed, frame_bytes);
  /* launch 0 feeds from the seed; launch t + 1 paints frame t and, unless it was the last, feeds from it */
  RamdAutomatonStep step = {.g = {ca->width, ca->height, d_off, ca->len_y, d_off + 2 * ca->len_y, ca->len_c, ca->len_pos,
                                  ca->edges},
                            .seed = d_seed, .hid0 = hid0, .row0 = rows.r0, .feed = 1};
  ramd_launch_automaton_step(ramd_stream, s, &e->b, &step);
  ramd_rows_forward(&rows, cells);
  step.seed = NULL;
  step.hid0 = NULL;
  size_t t0 = 0; /* the segment's first frame */
  for (size_t t = 0; t < (size_t)n_frames; t++) {
    const int last = t + 1 == (size_t)n_frames;
    const size_t slot = t - t0;
    step.paint = d_frames + slot * frame_bytes;
    step.feed = !last;
    ramd_launch_automaton_step(ramd_stream, s, &e->b, &step);
    if (!last) {
      ramd_rows_forward(&rows, cells);
    }
    if (slot + 1 == F || last) {
      ramd_d2h(frames + t0 * frame_bytes, d_frames, (slot + 1) * frame_bytes);
      if (last) { /* a row's last forward pass was its last writer */
        ramd_rows_states_out(&rows, cells, h_out);
      }
      ramd_dsync(); /* the segment's one synchronisation */
      t0 = t + 1;
    }
  }
  ramd_rows_close(&rows);
  return 0;
}
