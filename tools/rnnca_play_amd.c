/* rnnca_play_amd.c -- a trained rnnca net played as an automaton on the MI355X core: what the plugin's fill_frame
 * (gstrnnca.c:805-831) paints frame after frame, for many frames in ONE device call (rnn_amd_run_automaton).
 *
 * The plugin's host side -- GStreamer, the video sink, check_for_stasis and its generator -- is out of scope: the frames
 * go to a file as raw planar bytes, per frame the Y, the Cb and the Cr plane of W * H bytes each.
 *
 *   rnnca_play_amd [-w W] [-h H] [-p PATTERN] [-3] [-E] [-n FRAMES] [-s SEED | -i SEEDFILE] NET OUT
 *
 * -w, -h     the grid (default 144 x 96)
 * -p         the offset pattern (default "Y00120111C0111": 17 luma and 8 chroma neighbours)
 * -3         three position inputs instead of two
 * -E         wrapped edges instead of clamped ones
 * -n         frames to play (default 100)
 * -s         the seed frame is 3 * W * H bytes drawn from a generator seeded init_rand64(SEED) (recur-rng.h:33-43, the words
 *            stored as they lie in memory; default 1)
 * -i         the seed frame is the first 3 * W * H bytes of SEEDFILE */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "recur-nn.h"
#include "recur_amd.h"

#define MAX_PAIRS 512

/* Jenkins' small fast generator, 64 bit, as recur-rng.h seeds and steps it */
typedef struct Gen {
  u64 a, b, c, d;
} Gen;
static u64 rot(u64 x, int k) { return (x << k) | (x >> (64 - k)); }
static u64 gen_next(Gen *g) {
  const u64 e = g->a - rot(g->b, 7);
  g->a = g->b ^ rot(g->c, 13);
  g->b = g->c + rot(g->d, 37);
  g->c = g->d + e;
  g->d = e + g->a;
  return g->d;
}
static void gen_seed(Gen *g, u64 seed) {
  g->a = 0xf1ea5eed;
  g->b = g->c = g->d = seed;
  for (int i = 0; i < 20; i++) {
    gen_next(g);
  }
}

int main(int argc, char **argv) {
  int width = 144, height = 96, len_pos = 2, edges = 1, n_frames = 100, opt;
  const char *pattern = "Y00120111C0111", *seed_file = NULL;
  u64 seed_value = 1;
  while ((opt = getopt(argc, argv, "w:h:p:3En:s:i:")) != -1) {
    switch (opt) {
    case 'w': width = atoi(optarg); break;
    case 'h': height = atoi(optarg); break;
    case 'p': pattern = optarg; break;
    case '3': len_pos = 3; break;
    case 'E': edges = 0; break;
    case 'n': n_frames = atoi(optarg); break;
    case 's': seed_value = strtoull(optarg, NULL, 0); break;
    case 'i': seed_file = optarg; break;
    default: fprintf(stderr, "see the head of tools/rnnca_play_amd.c\n"); return 2;
    }
  }
  if (argc - optind != 2 || width < 1 || height < 1 || width > 0x7fffffff / 3 / height || n_frames < 0) {
    fprintf(stderr, "usage: rnnca_play_amd [-w W] [-h H] [-p PATTERN] [-3] [-E] [-n FRAMES] [-s SEED | -i SEEDFILE] NET OUT\n");
    return 2;
  }
  static int offsets_y[2 * MAX_PAIRS], offsets_c[2 * MAX_PAIRS];
  RnnAmdAutomaton ca = {.width = width, .height = height, .offsets_y = offsets_y, .offsets_c = offsets_c,
                        .len_pos = len_pos, .edges = edges};
  if (rnn_amd_automaton_parse_offsets(pattern, offsets_y, &ca.len_y, offsets_c, &ca.len_c, MAX_PAIRS)) {
    return 1;
  }
  RecurNN *net = rnn_load_net(argv[optind]);
  if (!net) {
    fprintf(stderr, "%s: not a net\n", argv[optind]);
    return 1;
  }
  const size_t frame_bytes = 3 * (size_t)width * height;
  u8 *seed = calloc(frame_bytes + sizeof(u64), 1);
  u8 *frames = malloc((size_t)n_frames * frame_bytes + 1);
  if (!seed || !frames) {
    fprintf(stderr, "out of memory for %d frames\n", n_frames);
    return 1;
  }
  if (seed_file) {
    FILE *f = fopen(seed_file, "rb");
    if (!f || fread(seed, 1, frame_bytes, f) != frame_bytes) {
      fprintf(stderr, "%s: no %zu bytes of a seed frame\n", seed_file, frame_bytes);
      return 1;
    }
    fclose(f);
  } else {
    Gen g;
    gen_seed(&g, seed_value);
    for (size_t i = 0; i < frame_bytes; i += sizeof(u64)) { /* (the buffer has a word to spare) */
      const u64 r = gen_next(&g);
      memcpy(seed + i, &r, sizeof r);
    }
  }
  if (rnn_amd_run_automaton(net, &ca, seed, n_frames, NULL, NULL, 0, frames)) {
    return 1;
  }
  FILE *out = fopen(argv[optind + 1], "wb");
  if (!out || fwrite(frames, 1, (size_t)n_frames * frame_bytes, out) != (size_t)n_frames * frame_bytes || fclose(out)) {
    perror(argv[optind + 1]);
    return 1;
  }
  free(seed);
  free(frames);
  rnn_delete_net(net);
  return 0;
}
