/* parrot_train_amd.c -- parrot's trainer on the MI355X core: what the plugin's maybe_learn (gstparrot.c:487-554) does per
 * chunk of audio -- every channel's net predicts the channel's next MDCT frame from the current one (train_net, 464-477),
 * then one update and rnn_condition_net -- for all channels at once and for a block of generations per device call
 * (rnn_amd_set_dense_steps_tanh): a frame is generation t's target and generation t + 1's input, so a block of frames goes
 * up once and nothing comes back but the progress figure.
 *
 * The plugin's host side -- GStreamer, the window, the MDCT -- is out of scope: the features come from a file.  The plugin
 * overwrites the delta sums channel by channel, so that only the last channel's reach the update; this trainer SUMS them
 * over the channels (include/recur_amd.h).  With -c 1 the two are the same.
 *
 *   parrot_train_amd [-c CHANNELS] [-H HIDDEN] [-d DEPTH] [-r RATE] [-m MOMENTUM] [-b BLOCK] [-s SEED] FEATURES NET
 *
 * FEATURES   raw float32 [frames][CHANNELS][256], the MDCT bins as the plugin scales them (within [-1, 1])
 * NET        where the trained net is saved (rnn_save_net): tools/parrot_dream_amd plays it
 * -c         channels (default 1)        -H  hidden size (default 199, the plugin's)
 * -d         BPTT depth (default 30)     -r  learn rate (default 0.0001)     -m  momentum (default 0.95)
 * -b         generations per device call (default 64)
 * -s         the net's seed (default 11, the plugin's)
 * The net is made as the plugin makes it (gstparrot.c:261-268): 256 / HIDDEN / 256, PARROT_RNN_FLAGS, RELU, no presynaptic
 * noise, rnn_randomise_weights_auto.  One line per block: the generations so far and the mean squared error per output of
 * the block, error / (count * 256) of rnn_amd_set_read_stats. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "recur-nn.h"
#include "recur_amd.h"

#define PARROT_N_FEATURES 256
#define PARROT_RNN_FLAGS (RNN_NET_FLAG_STANDARD | RNN_NET_FLAG_BPTT_ADAPTIVE_MIN_ERROR)

int main(int argc, char **argv) {
  int channels = 1, hidden = 199, depth = 30, block = 64, opt;
  float rate = 0.0001f, momentum = 0.95f;
  u64 seed = 11;
  while ((opt = getopt(argc, argv, "c:H:d:r:m:b:s:")) != -1) {
    switch (opt) {
    case 'c': channels = atoi(optarg); break;
    case 'H': hidden = atoi(optarg); break;
    case 'd': depth = atoi(optarg); break;
    case 'r': rate = strtof(optarg, NULL); break;
    case 'm': momentum = strtof(optarg, NULL); break;
    case 'b': block = atoi(optarg); break;
    case 's': seed = strtoull(optarg, NULL, 0); break;
    default: fprintf(stderr, "see the head of tools/parrot_train_amd.c\n"); return 2;
    }
  }
  if (argc - optind != 2 || channels < 1 || hidden < 1 || depth < 1 || block < 1) {
    fprintf(stderr, "usage: parrot_train_amd [-c CHANNELS] [-H HIDDEN] [-d DEPTH] [-r RATE] [-m MOMENTUM] [-b BLOCK] "
                    "[-s SEED] FEATURES NET\n");
    return 2;
  }
  FILE *in = fopen(argv[optind], "rb");
  if (!in || fseek(in, 0, SEEK_END)) {
    perror(argv[optind]);
    return 1;
  }
  const size_t frame = (size_t)channels * PARROT_N_FEATURES;
  const long n_frames = ftell(in) / (long)(frame * sizeof(float));
  rewind(in);
  if (n_frames < 2) {
    fprintf(stderr, "%s: fewer than 2 frames of %d channels\n", argv[optind], channels);
    return 1;
  }
  float *frames = malloc((size_t)n_frames * frame * sizeof(float));
  if (!frames || fread(frames, frame * sizeof(float), (size_t)n_frames, in) != (size_t)n_frames) {
    fprintf(stderr, "%s: could not read %ld frames\n", argv[optind], n_frames);
    return 1;
  }
  fclose(in);
  RecurNN *net = rnn_new(PARROT_N_FEATURES, hidden, PARROT_N_FEATURES, PARROT_RNN_FLAGS, seed, NULL, depth, rate, momentum,
                         0.0f, RNN_RELU);
  rnn_randomise_weights_auto(net);
  RecurNN **nets = rnn_new_training_set(net, channels);
  RnnAmdSet *set = rnn_amd_set_open(nets, channels);
  if (!set) {
    return 1;
  }
  RnnAmdStats st;
  rnn_amd_set_read_stats(set, &st, 1);
  /* the last frame of a block is the first of the next */
  for (long t = 0; t + 1 < n_frames; t += block) {
    const int steps = (int)(n_frames - 1 - t < block ? n_frames - 1 - t : block);
    rnn_amd_set_dense_steps_tanh(set, frames + (size_t)t * frame, PARROT_N_FEATURES, steps, PARROT_N_FEATURES,
                                 RNN_MOMENTUM_WEIGHTED, net->bptt->momentum, 1);
    rnn_amd_set_read_stats(set, &st, 1);
    printf("%ld %.9g\n", t + steps, st.error / ((double)st.count * PARROT_N_FEATURES));
    fflush(stdout);
  }
  rnn_amd_set_close(set);
  if (rnn_save_net(nets[0], argv[optind + 1], 0)) {
    fprintf(stderr, "%s: could not save the net\n", argv[optind + 1]);
    return 1;
  }
  free(frames);
  rnn_delete_training_set(nets, channels, 0);
  return 0;
}
