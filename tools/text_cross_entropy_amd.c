/* text_cross_entropy_amd.c -- what the reference's text-cross-entropy does
 * (text-cross-entropy.c:58-207; of the colour mode the xterm-256 form): load a net saved by a text
 * trainer, rebuild its alphabet from the net's metadata, and print the cross-entropy in bits
 * per character of each text file under the net's predictions.  The whole text runs
 * through the net on the device (rnn_char_cross_entropy -> rnn_amd_run_text).
 *
 *   text_cross_entropy_amd -f NET [-i ignore_first] [-m min_length] [-p prefix] [-I | -t | -c SCALE [-d DECAY]] TEXT...
 *
 * Like the reference, the plain form carries the net's state from one file into the next (and primes with the prefix
 * in front of every file), so a file's figure depends on the files before it.  -I (independent) scores every file on
 * its own from the state the net has after ONE priming with the prefix, all files in one batched device run
 * (rnn_amd_char_cross_entropy_texts); the lines and their order are the same.
 *
 * -t (trace) and -c (colour) score the files as -I does -- one priming, every file on its own -- through ONE
 * rnn_amd_trace_texts call for all files, and show where in a text the net was surprised:
 *   -t  one line per traced symbol in front of the file's `name entropy` line: name, the symbol's index in the encoded
 *       text, its code point, the bits it cost (-log2 p, all of a float's digits) and the code point of the net's best
 *       guess at it.  The entropy is the sum of the bits from index ignore_first + 1 on over len - ignore_first - 1,
 *       rnn_amd_char_cross_entropy_texts's expression.
 *   -c  the text itself, coloured by colourise_text's rule (text-cross-entropy.c:91-116): rolling starts at 1; every
 *       symbol from ignore_first + 1 on sets rolling = rolling * (1 - DECAY) + bits * DECAY and takes colour
 *       min(rolling * SCALE, colours - 1); an escape sequence is printed when the colour changes.  DECAY defaults to 1
 *       (no memory).  The palette is a ramp over the xterm-256 colour cube computed below, green to yellow to red to
 *       magenta.  The text is followed by a reset, a newline and the file's `name entropy` line.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "recur-nn.h"
#include "recur_amd_char.h"

#define USAGE "usage: %s -f NET [-i n] [-m n] [-p prefix] [-I | -t | -c scale [-d decay]] TEXT...\n"
#define N_COLOURS 16

/* colour k of the ramp as an index of the xterm-256 6 x 6 x 6 cube (16 + 36 r + 6 g + b): green, up the reds to yellow,
 * down the greens to red, up the blues to magenta */
static int ramp_colour(int k) {
  const int r = k < 5 ? k : 5, g = k < 6 ? 5 : (k < 11 ? 10 - k : 0), b = k < 11 ? 0 : k - 10;
  return 16 + 36 * r + 6 * g + b;
}

static void put_point(int point, int utf8) {
  if (!utf8 || point < 0x80) {
    putchar(point);
  } else if (point < 0x800) {
    putchar(0xC0 | (point >> 6));
    putchar(0x80 | (point & 0x3F));
  } else if (point < 0x10000) {
    putchar(0xE0 | (point >> 12));
    putchar(0x80 | ((point >> 6) & 0x3F));
    putchar(0x80 | (point & 0x3F));
  } else {
    putchar(0xF0 | (point >> 18));
    putchar(0x80 | ((point >> 12) & 0x3F));
    putchar(0x80 | ((point >> 6) & 0x3F));
    putchar(0x80 | (point & 0x3F));
  }
}

static int point_of(const RnnCharAlphabet *alphabet, int symbol) {
  return symbol < alphabet->len ? alphabet->points[symbol] : -1;
}

/* -t and -c: one priming, one traced run of all files, then the lines or the coloured text of each */
static int trace_files(RecurNN *net, RnnCharAlphabet *alphabet, u8 **texts, const int *lens, const char **names, int count,
                       int ignore_first, const u8 *prefix_text, int prefix_len, int colour, float scale, float decay) {
  float **logp = calloc(count + 1, sizeof(float *));
  u8 **guess = calloc(count + 1, sizeof(u8 *));
  for (int k = 0; k < count; k++) {
    logp[k] = calloc(lens[k] > 1 ? lens[k] - 1 : 1, sizeof(float));
    guess[k] = calloc(lens[k] > 1 ? lens[k] - 1 : 1, 1);
  }
  if (prefix_text) {
    rnn_char_prime(net, alphabet, prefix_text, prefix_len);
  }
  if (rnn_amd_trace_texts(net, (const u8 *const *)texts, lens, count, 0, logp, colour ? NULL : guess)) {
    return 1;
  }
  const int utf8 = (alphabet->flags & RNN_CHAR_FLAG_UTF8) != 0;
  for (int k = 0; k < count; k++) {
    double sum = 0.0;
    float rolling = 1.0f;
    int shown = -1;
    for (int i = 0; colour && i <= ignore_first && i < lens[k]; i++) {
      put_point(point_of(alphabet, texts[k][i]), utf8);
    }
    for (int t = 0; t < lens[k] - 1; t++) {
      const float bits = -logp[k][t];
      if (t >= ignore_first) {
        sum += (double)logp[k][t];
      }
      if (!colour) {
        printf("%s %d %d %.9g %d\n", names[k], t + 1, point_of(alphabet, texts[k][t + 1]), bits, point_of(alphabet, guess[k][t]));
      } else if (t >= ignore_first) {
        rolling = rolling * (1.0f - decay) + bits * decay;
        const float at = rolling * scale;
        const int index = at < (float)(N_COLOURS - 1) ? (at > 0.0f ? (int)at : 0) : N_COLOURS - 1;
        if (index != shown) {
          printf("\033[38;5;%dm", ramp_colour(index));
          shown = index;
        }
        put_point(point_of(alphabet, texts[k][t + 1]), utf8);
      }
    }
    if (colour) {
      printf("\033[0m\n");
    }
    printf("%s %.5f\n", names[k], sum / -(double)(lens[k] - ignore_first - 1));
    free(logp[k]);
    free(guess[k]);
  }
  free(logp);
  free(guess);
  return 0;
}

int main(int argc, char **argv) {
  const char *netfile = NULL, *prefix = NULL;
  int ignore_first = 0, min_length = 0, independent = 0, trace = 0, colour = 0, opt;
  float scale = 0.0f, decay = 1.0f;
  while ((opt = getopt(argc, argv, "f:i:m:p:Itc:d:")) != -1) {
    switch (opt) {
    case 't': trace = independent = 1; break;
    case 'c': scale = (float)atof(optarg); colour = independent = 1; break;
    case 'd': decay = (float)atof(optarg); break;
    case 'f': netfile = optarg; break;
    case 'i': ignore_first = atoi(optarg); break;
    case 'm': min_length = atoi(optarg); break;
    case 'p': prefix = optarg; break;
    case 'I': independent = 1; break;
    default: fprintf(stderr, USAGE, argv[0]); return 2;
    }
  }
  if (!netfile || optind >= argc || (trace && colour) || decay < 0.0f || decay > 1.0f) {
    fprintf(stderr, USAGE, argv[0]);
    return 2;
  }
  RecurNN *net = rnn_load_net(netfile);
  if (!net || !net->metadata) {
    fprintf(stderr, "'%s' is not a text net with metadata\n", netfile);
    return 1;
  }
  RnnCharAlphabet *alphabet = rnn_char_new_alphabet_from_net(net);
  int *char_to_net = rnn_char_new_char_lut(alphabet);
  u8 *prefix_text = NULL;
  int prefix_len = 0;
  if (prefix) {
    prefix_text = rnn_char_alloc_encoded_text(alphabet, prefix, (int)strlen(prefix), &prefix_len, NULL,
                                              false);
  }
  int count = 0;
  /* -I: the files are encoded first and scored together */
  u8 **texts = independent ? calloc(argc, sizeof(u8 *)) : NULL;
  int *lens = independent ? calloc(argc, sizeof(int)) : NULL;
  const char **names = independent ? calloc(argc, sizeof(char *)) : NULL;
  for (int i = optind; i < argc; i++) {
    char *raw;
    int raw_len;
    if (rnn_char_alloc_file_contents(argv[i], &raw, &raw_len)) {
      continue;
    }
    if (raw_len >= min_length && independent) {
      texts[count] = rnn_char_alloc_encoded_text(alphabet, raw, raw_len, &lens[count], char_to_net, false);
      names[count] = argv[i];
      count++;
    } else if (raw_len >= min_length) {
      int len;
      u8 *text = rnn_char_alloc_encoded_text(alphabet, raw, raw_len, &len, char_to_net, false);
      double entropy =
          rnn_char_cross_entropy(net, alphabet, text, len, ignore_first, prefix_text, prefix_len);
      printf("%s %.5f\n", argv[i], entropy);
      count++;
      free(text);
    }
    free(raw);
  }
  if (trace || colour) {
    if (trace_files(net, alphabet, texts, lens, names, count, ignore_first, prefix_text, prefix_len, colour, scale, decay)) {
      return 1;
    }
    for (int k = 0; k < count; k++) {
      free(texts[k]);
    }
    free(texts);
    free(lens);
    free(names);
  } else if (independent) {
    double *entropy = calloc(count + 1, sizeof(double));
    if (rnn_amd_char_cross_entropy_texts(net, alphabet, (const u8 *const *)texts, lens, count, ignore_first, prefix_text,
                                         prefix_len, entropy)) {
      return 1;
    }
    for (int k = 0; k < count; k++) {
      printf("%s %.5f\n", names[k], entropy[k]);
      free(texts[k]);
    }
    free(entropy);
    free(texts);
    free(lens);
    free(names);
  }
  free(char_to_net);
  free(prefix_text);
  rnn_char_free_alphabet(alphabet);
  rnn_delete_net(net);
  fprintf(stderr, "processed %d texts\n", count);
  return 0;
}
