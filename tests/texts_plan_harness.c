/* texts_plan_harness.c -- prints what recur_amd/csrc/texts_plan.h plans for the lengths, skips and wave width on its
 * command line (tests/test_texts_plan.py): built with the host compiler alone, no HIP.
 *
 *   texts_plan_harness WIDTH LEN,LEN,... [SKIP,SKIP,...]
 */
#include <stdio.h>
#include <string.h>
#include "texts_plan.h"

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
  static int lens[65536], skips[65536];
  if (argc < 3) return 2;
  const int width = atoi(argv[1]);
  const int n = parse_list(argv[2], lens, 65536);
  const int ns = argc > 3 ? parse_list(argv[3], skips, 65536) : 0;
  if (ns && ns != n) return 2;
  TextsPlan p;
  if (texts_plan_make(&p, lens, ns ? skips : NULL, n, width)) return 1;
  printf("n_rows=%d\nn_waves=%d\n", p.n_rows, p.n_waves);
  print_list("order", p.order, p.n_rows);
  print_list("len", p.len, p.n_rows);
  print_list("skip", p.skip, p.n_rows);
  for (int w = 0; w < p.n_waves; w++) {
    printf("wave%d=%d,%d,%d\n", w, p.waves[w].row0, p.waves[w].nrows, p.waves[w].steps);
    printf("active%d=", w);
    for (int t = 0; t <= p.waves[w].steps; t++) printf("%s%d", t ? "," : "", texts_plan_active(&p, w, t)); /* (one past the end: 0) */
    printf("\n");
  }
  texts_plan_free(&p);
  return 0;
}
