/* classify_run_amd.c -- a trained classifier net run over recordings' features on the MI355X core: what gstclassify's
 * emit_opinions (gstclassify.c:2259-2292) publishes per window, for many recordings in ONE batched device call
 * (rnn_amd_run_sequences).
 *
 * The plugin's host side -- GStreamer, FFT / MFCC features -- is out of scope: the features come from files, one per
 * recording, raw float32 [frames][net->input_size].  The class groups are the net's own: the `classes` item of its
 * metadata (rnn_amd_classify_load_metadata) through rnn_amd_classify_parse_classes.
 *
 *   classify_run_amd [-s segment_frames] NET FEATURES...
 *
 * prints, per file and window, one line:
 *   FILE WINDOW  then per class group: the winner's letter, and every class's probability (%.6f)
 * -s N stages N frames per row at a time (default: the library's). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "recur-nn.h"
#include "recur_amd_classify.h"

#define MAX_GROUPS 64

static float *read_features(const char *path, int width, int *frames) {
  FILE *f = fopen(path, "rb");
  if (!f) {
    perror(path);
    return NULL;
  }
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  const long row = (long)width * (long)sizeof(float);
  if (bytes < 0 || bytes % row != 0 || bytes / row > 0x7ffffffe) {
    fprintf(stderr, "%s: %ld bytes are not whole frames of %d floats\n", path, bytes, width);
    fclose(f);
    return NULL;
  }
  float *data = malloc(bytes ? (size_t)bytes : 1);
  if (!data || fread(data, 1, (size_t)bytes, f) != (size_t)bytes) {
    fprintf(stderr, "%s: could not be read\n", path);
    free(data);
    fclose(f);
    return NULL;
  }
  fclose(f);
  *frames = (int)(bytes / row);
  return data;
}

int main(int argc, char **argv) {
  int segment = 0, opt;
  while ((opt = getopt(argc, argv, "s:")) != -1) {
    switch (opt) {
    case 's': segment = atoi(optarg); break;
    default: fprintf(stderr, "see the head of tools/classify_run_amd.c\n"); return 2;
    }
  }
  if (argc - optind < 2) {
    fprintf(stderr, "usage: classify_run_amd [-s segment_frames] NET FEATURES...\n");
    return 2;
  }
  RecurNN *net = rnn_load_net(argv[optind]);
  if (!net) {
    fprintf(stderr, "%s: not a net\n", argv[optind]);
    return 1;
  }
  RnnAmdClassifyMetadata md = {0};
  if (rnn_amd_classify_load_metadata(net->metadata, &md) < 0 || !md.classes) {
    fprintf(stderr, "%s: no classifier metadata\n", argv[optind]);
    return 1;
  }
  int g_off[MAX_GROUPS], g_size[MAX_GROUPS], string_len = 0;
  const int n_groups = rnn_amd_classify_parse_classes(md.classes, g_off, g_size, MAX_GROUPS, NULL, &string_len);
  if (n_groups < 1 || n_groups > MAX_GROUPS || string_len > net->output_size) {
    fprintf(stderr, "%s: classes \"%s\" (%d groups) do not fit %d outputs\n", argv[optind], md.classes, n_groups,
            net->output_size);
    return 1;
  }
  const int n = argc - optind - 1, O = net->output_size;
  const float **inputs = calloc(n, sizeof(*inputs));
  float **answers = calloc(n, sizeof(*answers));
  u8 **winners = calloc(n, sizeof(*winners));
  int *frames = calloc(n, sizeof(int));
  for (int k = 0; k < n; k++) {
    inputs[k] = read_features(argv[optind + 1 + k], net->input_size, &frames[k]);
    if (!inputs[k]) {
      return 1;
    }
    answers[k] = malloc(((size_t)frames[k] * O + 1) * sizeof(float));
    winners[k] = malloc((size_t)frames[k] * n_groups + 1);
  }
  if (rnn_amd_run_sequences(net, inputs, frames, n, net->input_size, n_groups, g_off, g_size, NULL, NULL, segment,
                            (float *const *)answers, (u8 *const *)winners)) {
    return 1;
  }
  for (int k = 0; k < n; k++) {
    for (int t = 0; t < frames[k]; t++) {
      printf("%s %d", argv[optind + 1 + k], t);
      for (int g = 0; g < n_groups; g++) { /* (a group's offset is its place in the class string as well) */
        printf(" %c", md.classes[g_off[g] + winners[k][(size_t)t * n_groups + g]]);
        for (int i = 0; i < g_size[g]; i++) {
          printf(" %.6f", answers[k][(size_t)t * O + g_off[g] + i]);
        }
      }
      printf("\n");
    }
    free((void *)inputs[k]);
    free(answers[k]);
    free(winners[k]);
  }
  free(inputs); free(answers); free(winners); free(frames);
  rnn_amd_classify_free_metadata_items(&md);
  rnn_delete_net(net);
  return 0;
}
