/* text_classify_results_amd.c -- print, for each text file, the mean and the standard deviation of every class's
 * probability under a text classifier net (one that a text-classify style trainer saved, with its alphabet in the net's
 * metadata): a file's symbols run through the net one by one, the softmax over the class outputs is taken behind every
 * symbol, and the figures are taken over the symbols behind the first ignore_start.
 *
 *   text_classify_results_amd -f NET [-i ignore_start] [-m min_length] FILE...
 *
 * All files go through ONE rnn_amd_char_classify_texts call (include/recur_amd_char.h), side by side on the device.  One
 * line per file whose encoded text has at least min_length symbols (min_length is raised to ignore_start + 1):
 *
 *   FILE mean: %.3e ...  stddev: %.3e ...
 *
 * a figure per class in the order of the net's outputs.
 *
 * A documented difference from the reference's text-classify-results: that carries the net's state from one file into the
 * next, so a file's figures depend on the files before it.  Here EVERY file starts from the hidden row the net was saved
 * with, and the order of the files changes no figure.  (And the standard deviation is clamped at zero where the
 * reference's float arithmetic can print NaN: rnn_amd_char_classify_texts says how.) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "recur-nn.h"
#include "recur_amd_char.h"

#define USAGE "usage: %s -f NET [-i ignore_start] [-m min_length] FILE...\n"

int main(int argc, char **argv) {
  const char *netfile = NULL;
  int ignore_start = 0, min_length = 0, opt;
  while ((opt = getopt(argc, argv, "f:i:m:")) != -1) {
    switch (opt) {
    case 'f': netfile = optarg; break;
    case 'i': ignore_start = atoi(optarg); break;
    case 'm': min_length = atoi(optarg); break;
    default: fprintf(stderr, USAGE, argv[0]); return 2;
    }
  }
  if (!netfile || optind >= argc || ignore_start < 0) {
    fprintf(stderr, USAGE, argv[0]);
    return 2;
  }
  if (min_length <= ignore_start) {
    min_length = ignore_start + 1;
  }
  RecurNN *net = rnn_load_net(netfile);
  if (!net || !net->metadata) {
    fprintf(stderr, "'%s' is not a text net with metadata\n", netfile);
    return 1;
  }
  RnnCharAlphabet *alphabet = rnn_char_new_alphabet_from_net(net);
  int *char_to_net = rnn_char_new_char_lut(alphabet);
  char **raws = calloc(argc, sizeof(char *));
  int *bytes = calloc(argc, sizeof(int));
  const char **names = calloc(argc, sizeof(char *));
  int count = 0;
  for (int i = optind; i < argc; i++) {
    char *raw;
    int raw_len, len;
    if (rnn_char_alloc_file_contents(argv[i], &raw, &raw_len)) {
      continue;
    }
    free(rnn_char_alloc_encoded_text(alphabet, raw, raw_len, &len, char_to_net, false)); /* (for its length) */
    if (len < min_length) {
      free(raw);
      continue;
    }
    raws[count] = raw;
    bytes[count] = raw_len;
    names[count] = argv[i];
    count++;
  }
  const int n_out = net->output_size;
  double *mean = calloc((size_t)(count + 1) * n_out, sizeof(double));
  double *stddev = calloc((size_t)(count + 1) * n_out, sizeof(double));
  if (rnn_amd_char_classify_texts(net, alphabet, (const char *const *)raws, bytes, count, ignore_start, mean, stddev)) {
    return 1;
  }
  for (int k = 0; k < count; k++) {
    printf("%s mean: ", names[k]);
    for (int c = 0; c < n_out; c++) {
      printf("%.3e ", mean[(size_t)k * n_out + c]);
    }
    printf(" stddev: ");
    for (int c = 0; c < n_out; c++) {
      printf("%.3e ", stddev[(size_t)k * n_out + c]);
    }
    printf("\n");
    free(raws[k]);
  }
  free(mean);
  free(stddev);
  free(raws);
  free(bytes);
  free(names);
  free(char_to_net);
  rnn_char_free_alphabet(alphabet);
  rnn_delete_net(net);
  fprintf(stderr, "processed %d texts\n", count);
  return 0;
}
