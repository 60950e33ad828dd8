// continue_rule_harness.cpp -- prints what recur_amd/csrc/continue_rule.h says launch t = 0 .. plen + max_len does for a
// row with a prompt of plen symbols and max_len draws (tests/test_continue_rule.py): built with g++ alone, no HIP.
//
//   continue_rule_harness PLEN MAX_LEN        one line per launch: what,index,feeds,on_hid0
#include <cstdio>
#include <cstdlib>
#include "continue_rule.h"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  const int plen = atoi(argv[1]), max_len = atoi(argv[2]);
  for (int t = 0; t <= plen + max_len; t++) {
    const ContinueStep st = continue_step(plen, max_len, t);
    printf("%d,%d,%d,%d\n", st.what, st.index, st.feeds, st.on_hid0);
  }
  return 0;
}
