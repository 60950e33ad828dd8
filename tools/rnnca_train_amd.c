/* rnnca_train_amd.c -- rnnca's trainer on the MI355X core: what the plugin's maybe_learn (gstrnnca.c:718-750) does per video
 * frame -- every trainer predicts its own pixel of the frame now from its neighbourhood in the frame before (train_net,
 * 693-716), then one update and rnn_condition_net -- for all trainers at once and for a block of generations per device
 * call (rnn_amd_set_automaton_steps): a block of the film goes up once, the trainers' rows are gathered from its bytes on
 * the device, and nothing comes back but the progress figure.
 *
 * The plugin's host side -- GStreamer, the scaling of the video to the grid -- is out of scope: the film comes from a file.
 *
 *   rnnca_train_amd [-w W] [-h H] [-p PATTERN] [-3] [-E] [-t TRAINERS] [-H HIDDEN] [-d DEPTH] [-r RATE] [-m MOMENTUM]
 *                   [-S SOFT_START] [-b BLOCK] [-a] [-s SEED] FILM NET
 *
 * FILM       raw planar bytes [frames][3][H][W], the format tools/rnnca_play_amd writes
 * NET        where the trained net is saved (rnn_save_net): tools/rnnca_play_amd plays it
 * -w, -h     the grid (default 144 x 96)
 * -p         the offset pattern (default "Y00120111C0111")      -3  three position inputs instead of two
 * -E         wrapped edges instead of clamped ones (the plugin always trains clamped)
 * -t         trainers (default 200, the plugin's)               -H  hidden size (default 51, the plugin's)
 * -d         BPTT depth (default 10)     -r  learn rate (default 0.003)     -m  momentum (default 0.5)
 * -S         momentum soft start (default 0: none)              -b  generations per device call (default 64)
 * -a         advance every trainer's ring in front of its opinion (the plugin does not)
 * -s         the seed of the net and of the tool's own generator, which places the trainers (default 11)
 * The net is made as the plugin makes it (gstrnnca.c:326-331): inputs / HIDDEN / 3, the standard flags with the scaling
 * conditioner, RELU, no presynaptic noise.  The trainers are placed as construct_trainers and randomly_place_trainer place
 * them (gstrnnca.c:268-315): a margin of 2 cells from every edge (less on a grid too small for it), no two on one cell,
 * up to 20 draws each; after every 8th generation one trainer is moved (gstrnnca.c:743-748).  A block's positions are drawn
 * ahead and handed over per generation.  One line per block: the generations so far and the mean squared error per output
 * of the block, error / (count * 3) of rnn_amd_set_read_stats. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "recur-nn.h"
#include "recur_amd.h"

#define MAX_PAIRS 512
#define RNNCA_RNN_FLAGS (RNN_NET_FLAG_STANDARD | RNN_COND_USE_SCALE)
#define TRAINER_MARGIN 2
#define SHUFFLE_EVERY 8

/* Jenkins' small fast generator, 64 bit, as recur-rng.h seeds and steps it: the tool's own */
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

/* a free cell inside the margin for one trainer, marked in the mask: 0, or 1 after 20 draws that all hit a taken cell */
static int place_trainer(int *xy, Gen *g, u8 *mask, int w, int h) {
  const int mx = w > 2 * TRAINER_MARGIN ? TRAINER_MARGIN : 0, my = h > 2 * TRAINER_MARGIN ? TRAINER_MARGIN : 0;
  for (int i = 0; i < 20; i++) {
    const int x = mx + (int)(gen_next(g) % (u64)(w - 2 * mx));
    const int y = my + (int)(gen_next(g) % (u64)(h - 2 * my));
    if (!mask[y * w + x]) {
      mask[y * w + x] = 255;
      xy[0] = x;
      xy[1] = y;
      return 0;
    }
  }
  return 1;
}

int main(int argc, char **argv) {
  int width = 144, height = 96, len_pos = 2, edges = 1, trainers = 200, hidden = 51, depth = 10, block = 64, advance = 0, opt;
  float rate = 0.003f, momentum = 0.5f, soft_start = 0.0f;
  const char *pattern = "Y00120111C0111";
  u64 seed = 11;
  while ((opt = getopt(argc, argv, "w:h:p:3Et:H:d:r:m:S:b:as:")) != -1) {
    switch (opt) {
    case 'w': width = atoi(optarg); break;
    case 'h': height = atoi(optarg); break;
    case 'p': pattern = optarg; break;
    case '3': len_pos = 3; break;
    case 'E': edges = 0; break;
    case 't': trainers = atoi(optarg); break;
    case 'H': hidden = atoi(optarg); break;
    case 'd': depth = atoi(optarg); break;
    case 'r': rate = strtof(optarg, NULL); break;
    case 'm': momentum = strtof(optarg, NULL); break;
    case 'S': soft_start = strtof(optarg, NULL); break;
    case 'b': block = atoi(optarg); break;
    case 'a': advance = 1; break;
    case 's': seed = strtoull(optarg, NULL, 0); break;
    default: fprintf(stderr, "see the head of tools/rnnca_train_amd.c\n"); return 2;
    }
  }
  if (argc - optind != 2 || width < 1 || height < 1 || width > 0x7fffffff / 3 / height || trainers < 1 || hidden < 1 ||
      depth < 1 || block < 1) {
    fprintf(stderr, "usage: rnnca_train_amd [-w W] [-h H] [-p PATTERN] [-3] [-E] [-t TRAINERS] [-H HIDDEN] [-d DEPTH] [-r RATE] "
                    "[-m MOMENTUM] [-S SOFT_START] [-b BLOCK] [-a] [-s SEED] FILM NET\n");
    return 2;
  }
  static int offsets_y[2 * MAX_PAIRS], offsets_c[2 * MAX_PAIRS];
  RnnAmdAutomaton ca = {.width = width, .height = height, .offsets_y = offsets_y, .offsets_c = offsets_c,
                        .len_pos = len_pos, .edges = edges};
  if (rnn_amd_automaton_parse_offsets(pattern, offsets_y, &ca.len_y, offsets_c, &ca.len_c, MAX_PAIRS)) {
    return 1;
  }
  FILE *in = fopen(argv[optind], "rb");
  if (!in || fseek(in, 0, SEEK_END)) {
    perror(argv[optind]);
    return 1;
  }
  const size_t frame = 3 * (size_t)width * height;
  const long n_frames = ftell(in) / (long)frame;
  rewind(in);
  if (n_frames < 2) {
    fprintf(stderr, "%s: fewer than 2 frames of %d x %d\n", argv[optind], width, height);
    return 1;
  }
  u8 *film = malloc((size_t)n_frames * frame);
  if (!film || fread(film, frame, (size_t)n_frames, in) != (size_t)n_frames) {
    fprintf(stderr, "%s: could not read %ld frames\n", argv[optind], n_frames);
    return 1;
  }
  fclose(in);
  /* the trainers' places */
  Gen g;
  gen_seed(&g, seed);
  u8 *mask = calloc((size_t)width * height, 1);
  int *now = malloc(2 * (size_t)trainers * sizeof(int));
  int *xy = malloc(2 * (size_t)trainers * (size_t)block * sizeof(int));
  if (!mask || !now || !xy) {
    fprintf(stderr, "out of memory for %d trainers\n", trainers);
    return 1;
  }
  int placed = 0;
  for (int i = 0; i < 2 * trainers && placed < trainers; i++) {
    placed += !place_trainer(now + 2 * placed, &g, mask, width, height);
  }
  if (placed < trainers) {
    fprintf(stderr, "could only fit %d of %d trainers on %d x %d\n", placed, trainers, width, height);
    return 1;
  }
  RecurNN *net = rnn_new(ca.len_y + 2 * ca.len_c + len_pos, hidden, 3, RNNCA_RNN_FLAGS, seed, NULL, depth, rate, momentum, 0.0f,
                         RNN_RELU);
  rnn_randomise_weights_auto(net);
  RecurNN **nets = rnn_new_training_set(net, trainers);
  RnnAmdSet *set = rnn_amd_set_open(nets, trainers);
  if (!set) {
    return 1;
  }
  RnnAmdStats st;
  rnn_amd_set_read_stats(set, &st, 1);
  long generation = 0;
  /* the last frame of a block is the first of the next */
  for (long t = 0; t + 1 < n_frames; t += block) {
    const int steps = (int)(n_frames - 1 - t < block ? n_frames - 1 - t : block);
    for (int k = 0; k < steps; k++) { /* generation k trains where the trainers stand; behind every 8th one is moved */
      memcpy(xy + 2 * (size_t)k * trainers, now, 2 * (size_t)trainers * sizeof(int));
      generation++;
      if (generation % SHUFFLE_EVERY == 0) {
        int *one = now + 2 * (gen_next(&g) % (u64)trainers);
        mask[one[1] * width + one[0]] = 0;
        if (place_trainer(one, &g, mask, width, height)) {
          mask[one[1] * width + one[0]] = 255; /* (no free cell found: it stays) */
        }
      }
    }
    rnn_amd_set_automaton_steps(set, &ca, film + (size_t)t * frame, xy, 1, steps, advance, RNN_MOMENTUM_WEIGHTED, momentum,
                                soft_start, 1);
    rnn_amd_set_read_stats(set, &st, 1);
    printf("%ld %.9g\n", t + steps, st.error / ((double)st.count * 3));
    fflush(stdout);
  }
  rnn_amd_set_close(set);
  if (rnn_save_net(nets[0], argv[optind + 1], 0)) {
    fprintf(stderr, "%s: could not save the net\n", argv[optind + 1]);
    return 1;
  }
  free(film);
  free(mask);
  free(now);
  free(xy);
  rnn_delete_training_set(nets, trainers, 0);
  return 0;
}
