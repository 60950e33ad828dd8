// noise_ahead_harness.cpp -- recur_amd/csrc/noise_ahead.h under the host compiler alone, for tests/test_noise_ahead.py:
// the rule by which a forward pass takes the noise that was generated ahead of it, asked on the CPU.
//
//   noise_ahead_harness MODE < events      MODE: RECUR_AMD_NOISE_AHEAD's, 0 off, 1 one pass ahead, otherwise two
//
// One event per line of the input, one line of answer for each:
//   write                         a generator was written from the host
//   pass R0 N LEVEL BOTTOM        a forward pass of state rows [R0, R0 + N)      -> took=<slot | -1>
//   offer ROW0 N LEVEL CLASSES    an offer to generate ahead (CLASSES 0: plain)  -> behind_main=<0 | 1> and per launch
//                                 launch=<dst>,<src | -1>,<n_classes>,<skip>,<version>,<assumed_classes>
//   classes HEADS C0 C1 ...       the streams' classes were uploaded for a loss of HEADS heads
//   loss HEADS                    the multi-head loss ran                         -> dropped=<0 | 1>
//   free                          the device image was freed
// Every answer ends with the state the event left: moves=<count> head=<slot> adopted=<slot | -1> in_range=<0 | 1> and
// pending=<p0><p1>.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>
#include "noise_ahead.h"

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s MODE < events\n", argv[0]);
    return 2;
  }
  const int mode = atoi(argv[1]);
  NoiseAhead a;
  noise_ahead_reset(&a);
  char line[4096];
  while (fgets(line, sizeof line, stdin)) {
    std::istringstream in(line);
    std::string what;
    if (!(in >> what)) {
      continue;
    }
    printf("%s", what.c_str());
    if (what == "write") {
      noise_ahead_host_write(&a);
    } else if (what == "pass") {
      int r0, n, bottom;
      float level;
      in >> r0 >> n >> level >> bottom;
      printf(" took=%d", noise_ahead_pass(&a, r0, n, level, bottom));
    } else if (what == "offer") {
      int row0, n, classes;
      float level;
      in >> row0 >> n >> level >> classes;
      const NoiseAheadPlan p = noise_ahead_offer(&a, row0, n, level, classes, mode);
      printf(" behind_main=%d", p.behind_main);
      for (int i = 0; i < p.n_launches; i++) {
        const NoiseAheadLaunch &l = p.launch[i];
        printf(" launch=%d,%d,%d,%d,%lu,%d", l.dst, l.src, l.n_classes, l.skip, l.version, l.assumed_classes);
      }
    } else if (what == "classes") {
      int heads, c;
      std::vector<int> classes;
      in >> heads;
      while (in >> c) {
        classes.push_back(c);
      }
      noise_ahead_classes(&a, classes.data(), (int)classes.size(), heads);
    } else if (what == "loss") {
      int heads;
      in >> heads;
      printf(" dropped=%d", noise_ahead_loss(&a, heads));
    } else if (what == "free") {
      noise_ahead_freed(&a);
    } else {
      fprintf(stderr, "%s: no such event\n", what.c_str());
      return 2;
    }
    if (in.fail() && !in.eof()) {
      fprintf(stderr, "cannot read: %s", line);
      return 2;
    }
    printf(" moves=%lu head=%d adopted=%d in_range=%d pending=%d%d\n", a.moves, a.head, a.adopted, a.classes_in_range,
           a.slot[0].pending, a.slot[1].pending);
    fflush(stdout); /* (the test asks event by event: what a caller does next depends on the answer) */
  }
  return 0;
}
