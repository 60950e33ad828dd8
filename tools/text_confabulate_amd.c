/* text_confabulate_amd.c -- what the reference's text-confabulate does
 * (text-confabulate.c:50-103): load a text net, optionally prime it with a prefix, and
 * sample characters from its predictions.
 *
 *   text_confabulate_amd -f NET [-B bias] [-n chars] [-p prefix] [-u until_char]
 *                        [-w wait_for_char] [-r seed] [-N passages] [-P prompts_file [-e]]
 *
 * -N n: n passages, one per line, each from the (primed) net's state with a generator of its own seeded seed, seed + 1,
 * ..., all drawn in one batched device run (rnn_amd_char_confabulate_texts).  Without -N the one passage is drawn with the
 * net's own generator, as ever.  -w has no batched form (priming is what brings a net to a starting point).
 * -P FILE: every non-empty line of FILE is a prompt, continued n times (-N n, default 1) from the (primed) net's state:
 * lines x n rows in one batched device run (rnn_amd_char_continue_texts), row i -- the lines in order, a line's n
 * continuations next to one another -- with a generator seeded seed + i.  One output line per row: the prompt, then its
 * continuation.  -P does not go with -w either.
 * -P FILE -e: the same lines, each also scored: every prompt is fed once, scored on its way, and continued n times from the
 * state behind it (rnn_amd_char_score_and_continue_texts).  Every output line is prefixed by its prompt's bits per symbol
 * and a tab.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "recur-nn.h"
#include "recur_amd_char.h"

/* init_rand64 of recur-rng.h:33-43: callers of the reference seed net->rng themselves
 * (text-confabulate.c:67) */
static void seed_rng(rand_ctx *x, u64 seed) {
  x->a = 0xf1ea5eed;
  x->b = x->c = x->d = seed;
  for (int i = 0; i < 20; i++) {
    u64 e = x->a - ((x->b << 7) | (x->b >> 57));
    x->a = x->b ^ ((x->c << 13) | (x->c >> 51));
    x->b = x->c + ((x->d << 37) | (x->d >> 27));
    x->c = x->d + e;
    x->d = e + x->a;
  }
}

/* -P: the non-empty lines of `file` n times over, continued in one call; one line per row on stdout */
static int continue_prompts(RecurNN *net, RnnCharAlphabet *alphabet, const char *file, int n, long long seed, int chars,
                            float bias, int stop_point, int byte_len, int scored) {
  FILE *f = fopen(file, "r");
  if (!f) {
    fprintf(stderr, "cannot read the prompts in %s\n", file);
    return 1;
  }
  char **prompts = NULL, *line = NULL;
  size_t cap = 0, n_lines = 0;
  ssize_t got;
  while ((got = getline(&line, &cap, f)) >= 0) {
    while (got > 0 && (line[got - 1] == '\n' || line[got - 1] == '\r')) {
      line[--got] = 0;
    }
    if (got > 0) {
      prompts = realloc(prompts, sizeof(char *) * (n_lines + 1));
      prompts[n_lines++] = strdup(line);
    }
  }
  free(line);
  fclose(f);
  const int rows = (int)n_lines * n;
  const char **of_row = malloc(sizeof(char *) * (rows + 1));
  int *prompt_bytes = malloc(sizeof(int) * (rows + 1));
  u64 *seeds = malloc(sizeof(u64) * (rows + 1));
  char **lines = malloc(sizeof(char *) * (rows + 1));
  int *bytes = malloc(sizeof(int) * (rows + 1));
  for (int i = 0; i < rows; i++) {
    of_row[i] = prompts[i / n];
    prompt_bytes[i] = (int)strlen(of_row[i]);
    seeds[i] = (u64)seed + (u64)i;
    lines[i] = malloc(byte_len);
  }
  double *entropy = calloc(n_lines + 1, sizeof(double));
  int r;
  if (scored) { /* a prompt per line, not per row: each is fed once */
    for (size_t l = 0; l < n_lines; l++) {
      prompt_bytes[l] = (int)strlen(prompts[l]);
    }
    r = n < 1 ? 0 : rnn_amd_char_score_and_continue_texts(net, alphabet, (const char *const *)prompts, prompt_bytes, seeds,
                                                          (int)n_lines, n, chars, bias, stop_point, lines, byte_len, bytes,
                                                          entropy);
  } else {
    r = rnn_amd_char_continue_texts(net, alphabet, of_row, prompt_bytes, seeds, rows, chars, bias, stop_point, lines,
                                    byte_len, bytes);
  }
  for (int i = 0; i < rows; i++) {
    if (r == 0) {
      if (scored) {
        printf("%.6f\t", entropy[i / n]);
      }
      fputs(of_row[i], stdout);
      fputs(lines[i], stdout);
      fputs("\n", stdout);
    }
    free(lines[i]);
  }
  for (size_t l = 0; l < n_lines; l++) {
    free(prompts[l]);
  }
  free(prompts);
  free(of_row);
  free(prompt_bytes);
  free(seeds);
  free(lines);
  free(bytes);
  free(entropy);
  return r ? 1 : 0;
}

int main(int argc, char **argv) {
  const char *netfile = NULL, *prefix = NULL, *until = NULL, *wait_for = NULL, *prompts_file = NULL;
  float bias = 0;
  int chars = 72, opt, passages = -1, scored = 0;
  long long seed = 2;
  while ((opt = getopt(argc, argv, "f:B:n:p:u:w:r:N:P:e")) != -1) {
    switch (opt) {
    case 'f': netfile = optarg; break;
    case 'B': bias = atof(optarg); break;
    case 'n': chars = atoi(optarg); break;
    case 'p': prefix = optarg; break;
    case 'u': until = optarg; break;
    case 'w': wait_for = optarg; break;
    case 'r': seed = atoll(optarg); break;
    case 'N': passages = atoi(optarg); break;
    case 'P': prompts_file = optarg; break;
    case 'e': scored = 1; break;
    default: fprintf(stderr, "usage: %s -f NET [-B bias] [-n chars] [-p prefix]\n", argv[0]); return 2;
    }
  }
  if ((passages >= 0 || prompts_file) && wait_for) {
    fprintf(stderr, "usage: %s -f NET [-N passages] [-P prompts_file] [-B bias] [-n chars] [-p prefix] [-u until_char] "
                    "[-r seed]: -w does not go with -N or -P\n", argv[0]);
    return 2;
  }
  RecurNN *net = netfile ? rnn_load_net(netfile) : NULL;
  if (!net || !net->metadata) {
    fprintf(stderr, "need -f NET (a text net with metadata)\n");
    return 1;
  }
  RnnCharAlphabet *alphabet = rnn_char_new_alphabet_from_net(net);
  seed_rng(&net->rng, (u64)seed);
  rnn_amd_host_written(net, RNN_AMD_STREAM);
  int prev_char = 0;
  if (prefix) {
    int prefix_len;
    u8 *prefix_text = rnn_char_alloc_encoded_text(alphabet, prefix, (int)strlen(prefix), &prefix_len,
                                                  NULL, false);
    prev_char = rnn_char_prime(net, alphabet, prefix_text, prefix_len);
    free(prefix_text);
  }
  int byte_len = chars * 4 + 5;
  char *t = malloc(byte_len);
  int stop_point = until ? rnn_char_get_codepoint(alphabet, until) : -1;
  int start_point = wait_for ? rnn_char_get_codepoint(alphabet, wait_for) : -1;
  if (prompts_file) {
    int r = continue_prompts(net, alphabet, prompts_file, passages >= 0 ? passages : 1, seed, chars, bias, stop_point, byte_len,
                             scored);
    free(t);
    rnn_char_free_alphabet(alphabet);
    rnn_delete_net(net);
    return r;
  }
  if (passages >= 0) {
    u64 *seeds = malloc(sizeof(u64) * (passages + 1));
    char **lines = malloc(sizeof(char *) * (passages + 1));
    int *bytes = malloc(sizeof(int) * (passages + 1));
    for (int k = 0; k < passages; k++) {
      seeds[k] = (u64)seed + (u64)k;
      lines[k] = malloc(byte_len);
    }
    int r = rnn_amd_char_confabulate_texts(net, alphabet, seeds, passages, chars, bias, prev_char, stop_point, lines,
                                           byte_len, bytes);
    for (int k = 0; k < passages; k++) {
      fputs(lines[k], stdout);
      fputs("\n", stdout);
      free(lines[k]);
    }
    free(seeds);
    free(lines);
    free(bytes);
    free(t);
    rnn_char_free_alphabet(alphabet);
    rnn_delete_net(net);
    return r ? 1 : 0;
  }
  rnn_char_confabulate(net, t, chars, byte_len, alphabet, bias, &prev_char, start_point, stop_point);
  fputs(t, stdout);
  fputs("\n", stdout);
  free(t);
  rnn_char_free_alphabet(alphabet);
  rnn_delete_net(net);
  return 0;
}
