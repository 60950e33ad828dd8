/* parrot_dream_amd.c -- a trained parrot net dreaming on the MI355X core: what the plugin's player (fill_audio_chunk,
 * gstparrot.c:556-583) makes of every channel's dream net, frame after frame, for many channels and many frames in ONE
 * device call (rnn_amd_dream_sequences).
 *
 * The plugin's host side -- GStreamer, the MDCT synthesis, the overlap-add and the s16 samples -- is out of scope: the
 * frames go to a file as raw float32, per frame CHANNELS rows of the net's output_size values (the tanh answers, before
 * the noise).
 *
 *   parrot_dream_amd [-c CHANNELS] [-n FRAMES] [-s SEED] [-z NOISE] NET OUT
 *
 * -c         channels, each a clone of the net with a generator of its own (default 1)
 * -n         frames to dream (default 100)
 * -s         channel k's generator is init_rand64(SEED + k) (default 1)
 * -z         the noise level: an answer is multiplied by 1 + NOISE * cheap_gaussian_noise before it is fed back
 *            (default 1, the plugin's; 0 draws nothing)
 * Every channel starts from a zero row, as a fresh dream_net->output_layer is, on the net's hidden row. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "recur-nn.h"
#include "recur_amd.h"

int main(int argc, char **argv) {
  int channels = 1, n_frames = 100, opt;
  u64 seed = 1;
  float noise = 1.0f;
  while ((opt = getopt(argc, argv, "c:n:s:z:")) != -1) {
    switch (opt) {
    case 'c': channels = atoi(optarg); break;
    case 'n': n_frames = atoi(optarg); break;
    case 's': seed = strtoull(optarg, NULL, 0); break;
    case 'z': noise = strtof(optarg, NULL); break;
    default: fprintf(stderr, "see the head of tools/parrot_dream_amd.c\n"); return 2;
    }
  }
  if (argc - optind != 2 || channels < 1 || n_frames < 0) {
    fprintf(stderr, "usage: parrot_dream_amd [-c CHANNELS] [-n FRAMES] [-s SEED] [-z NOISE] NET OUT\n");
    return 2;
  }
  RecurNN *net = rnn_load_net(argv[optind]);
  if (!net) {
    fprintf(stderr, "%s: not a net\n", argv[optind]);
    return 1;
  }
  const size_t row = (size_t)(net->input_size > net->output_size ? net->input_size : net->output_size);
  const size_t count = (size_t)n_frames * (size_t)channels * (size_t)net->output_size;
  float *first = calloc((size_t)channels * row, sizeof(float));
  float *frames = malloc((count + 1) * sizeof(float));
  u64 *seeds = malloc((size_t)channels * sizeof(u64));
  if (!first || !frames || !seeds) {
    fprintf(stderr, "out of memory for %d frames of %d channels\n", n_frames, channels);
    return 1;
  }
  for (int k = 0; k < channels; k++) {
    seeds[k] = seed + (u64)k;
  }
  if (rnn_amd_dream_sequences(net, first, (int)row, channels, n_frames, noise, seeds, NULL, NULL, NULL, 0, frames, NULL,
                              NULL)) {
    return 1;
  }
  FILE *out = fopen(argv[optind + 1], "wb");
  if (!out || fwrite(frames, sizeof(float), count, out) != count || fclose(out)) {
    perror(argv[optind + 1]);
    return 1;
  }
  free(first);
  free(frames);
  free(seeds);
  rnn_delete_net(net);
  return 0;
}
