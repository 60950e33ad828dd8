/* seqs_plan_harness.cpp -- prints what recur_amd/csrc/seqs_plan.h plans for the frame counts, wave width and segment
 * length on its command line (tests/test_seqs_plan.py), and stages every frame through buffers of exactly the size the
 * plan says: built with the host compiler alone, no HIP; the same program runs under the sanitizers.
 *
 *   seqs_plan_harness WIDTH SEGMENT_FRAMES INPUT_SIZE FRAMES,FRAMES,...
 *
 * The staging is the call's, with one int where that has a frame, an answer row and a winner row: per segment every live
 * row's frames are written at off[j] + i of a buffer of seqs_plan_largest() ints ("upload"), read back from there
 * ("copy back") and counted at (caller's sequence, frame).  hits=lowest,highest count over all frames of all sequences. */
#include <stdio.h>
#include <string.h>
#include <vector>
#include "seqs_plan.h"

static int parse_list(const char *s, int *out, int cap) {
  int n = 0;
  while (*s && n < cap) {
    out[n++] = (int)strtol(s, (char **)&s, 10);
    if (*s == ',') s++;
  }
  return n;
}

static void print_list(const char *name, const int *v, int n) {
  printf("%s=", name);
  for (int i = 0; i < n; i++) printf("%s%d", i ? "," : "", v[i]);
  printf("\n");
}

int main(int argc, char **argv) {
  static int frames[65536];
  if (argc < 5) return 2;
  const int width = atoi(argv[1]), asked = atoi(argv[2]), input_size = atoi(argv[3]);
  const int n = parse_list(argv[4], frames, 65536);
  const int F = seqs_plan_segment_frames(asked, input_size, width);
  printf("segment=%d\ndefault=%d\n", F, seqs_plan_default_segment(input_size, width));
  TextsPlan p;
  std::vector<int> lens(n);
  if (seqs_plan_make(&p, frames, n, width, lens.data())) return 1;
  for (int k = 0; k < n; k++)
    if (lens[k] != frames[k] + 1) return 6;
  printf("n_rows=%d\nn_waves=%d\n", p.n_rows, p.n_waves);
  print_list("order", p.order, p.n_rows);
  std::vector<int> row_frames(p.n_rows);
  for (int r = 0; r < p.n_rows; r++) row_frames[r] = p.len[r] - 1;
  print_list("frames", row_frames.data(), p.n_rows);
  const unsigned long long largest = seqs_plan_largest(&p, F);
  printf("largest=%llu\n", largest);
  std::vector<int> staging(largest); /* exactly the plan's room: a slot beyond it is the sanitizer's to find */
  std::vector<std::vector<int>> hits(n);
  for (int k = 0; k < n; k++) hits[k].assign(frames[k], 0);
  for (int w = 0; w < p.n_waves; w++) {
    const TextsWave *wave = &p.waves[w];
    printf("wave%d=%d,%d,%d\n", w, wave->row0, wave->nrows, wave->steps);
    const int nseg = seqs_plan_segments(&p, w, F);
    printf("segments%d=%d\n", w, nseg);
    std::vector<int> count(wave->nrows);
    std::vector<unsigned long long> off(wave->nrows);
    for (int q = 0; q < nseg; q++) {
      int t0, len, live;
      const unsigned long long total = seqs_plan_segment(&p, w, q, F, &t0, &len, &live, count.data(), off.data());
      printf("seg%d_%d=%d,%d,%d,%llu\n", w, q, t0, len, live, total);
      char name[64];
      snprintf(name, sizeof name, "count%d_%d", w, q);
      print_list(name, count.data(), wave->nrows);
      printf("off%d_%d=", w, q);
      for (int j = 0; j < wave->nrows; j++) printf("%s%llu", j ? "," : "", off[j]);
      printf("\n");
      if (total > largest) return 3;
      for (int j = 0; j < live; j++) /* "upload": the frame's number within its sequence, tagged with the row */
        for (int i = 0; i < count[j]; i++) staging[off[j] + i] = (wave->row0 + j) * 100000 + t0 + i;
      for (int i = 0; i <= len; i++) { /* the launches: the rows fed at frame t0 + i are scored at the next launch */
        const int a = i < len ? texts_plan_active(&p, w, t0 + i) : 0;
        for (int j = 0; j < a; j++)
          if (i >= count[j]) return 4; /* a row that runs has the frame staged */
      }
      for (int j = 0; j < live; j++) /* "copy back" */
        for (int i = 0; i < count[j]; i++) {
          const int tag = staging[off[j] + i];
          if (tag != (wave->row0 + j) * 100000 + t0 + i) return 5; /* another row wrote the slot */
          hits[p.order[wave->row0 + j]][t0 + i]++;
        }
    }
  }
  int lo = 0x7fffffff, hi = 0;
  for (int k = 0; k < n; k++)
    for (int t = 0; t < frames[k]; t++) {
      lo = hits[k][t] < lo ? hits[k][t] : lo;
      hi = hits[k][t] > hi ? hits[k][t] : hi;
    }
  if (hi == 0) lo = 0;
  printf("hits=%d,%d\n", lo, hi);
  texts_plan_free(&p);
  return 0;
}
