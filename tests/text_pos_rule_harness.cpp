// Asks recur_amd/csrc/text_pos_rule.h where a stream reads the text and compares every answer with the reference's
// statement, (i + stream * spacing) % (len - 1) (tests/test_text_pos_rule.py).  Host code only.
//   sweep lo hi        every len in lo..hi, global_count in 1..len + 2, stream in 0..global_count - 1, i in 0..len - 1
//   at len count i ... every stream of `count` at the given positions
//   one len count stream i   prints offset=...
// sweep / at print cases=N bad=M and the first mismatches; exit status 1 where there is one.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "text_pos_rule.h"

static long cases = 0, bad = 0;

static void one(int len, int count, int stream, int i) {
  const int o = text_pos(len, count, stream, i);
  const long spacing = (len - 1) / count;
  const long want = ((long)i + (long)stream * spacing) % (len - 1);
  cases++;
  if (o != want || !(o >= 0 && o + 1 < len)) {
    if (bad++ < 10) printf("mismatch len=%d count=%d stream=%d i=%d: %d, want %ld\n", len, count, stream, i, o, want);
  }
}

int main(int argc, char **argv) {
  if (argc == 4 && !strcmp(argv[1], "sweep")) {
    for (int len = atoi(argv[2]); len <= atoi(argv[3]); len++)
      for (int count = 1; count <= len + 2; count++)
        for (int stream = 0; stream < count; stream++)
          for (int i = 0; i <= len - 1; i++) one(len, count, stream, i);
  } else if (argc >= 5 && !strcmp(argv[1], "at")) {
    const int len = atoi(argv[2]), count = atoi(argv[3]);
    for (int a = 4; a < argc; a++)
      for (int stream = 0; stream < count; stream++) one(len, count, stream, atoi(argv[a]));
  } else if (argc == 6 && !strcmp(argv[1], "one")) {
    printf("offset=%d\n", text_pos(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5])));
    return 0;
  } else {
    return fprintf(stderr, "usage: sweep lo hi | at len count i ... | one len count stream i\n"), 2;
  }
  printf("cases=%ld\nbad=%ld\n", cases, bad);
  return bad ? 1 : 0;
}
