// Prints what recur_amd/csrc/chain_plan.h says about the early form of the one-launch chain (chain_early_blocks, and the
// `early` field of every segment of a call's plan) as key=value lines (tests/test_chain_early_plan.py).  Arguments are
// key=value too; the switch comes from the environment.  Host code only.
#include <map>
#include <string>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "chain_plan.h"

int env_int(const char *name, int dflt) {
  const char *e = getenv(name);
  return (e && *e) ? atoi(e) : dflt;
}

int main(int argc, char **argv) {
  std::map<std::string, long long> a = {{"hidden", 1024}, {"nrows", 256}, {"depth", 20}, {"row0", 0}, {"scap", -1}};
  for (int i = 1; i < argc; i++) {
    const char *eq = strchr(argv[i], '=');
    std::string key(argv[i], eq ? eq - argv[i] : strlen(argv[i]));
    if (!eq || !a.count(key)) return fprintf(stderr, "unknown argument %s\n", argv[i]), 2;
    a[key] = strtoll(eq + 1, nullptr, 0);
  }
  const int hidden = (int)a["hidden"];
  printf("blocks=%d\n", PC_EARLY);
  printf("rule_full=%d\nrule_one=%d\nrule_pad=%d\n", chain_early_blocks(hidden, false, false), chain_early_blocks(hidden, true, false),
         chain_early_blocks(hidden, true, true));
  RamdShape sh = {};
  sh.input_size = sh.output_size = 42, sh.hidden_size = hidden;
  sh.I = (1 + sh.input_size + sh.hidden_size + 3) & ~3, sh.H = (sh.hidden_size + 1 + 3) & ~3, sh.O = (sh.output_size + 3) & ~3;
  sh.D = (int)a["depth"], sh.activation = 1;
  const int row0 = (int)a["row0"], nrows = (int)a["nrows"];
  sh.Scap = a["scap"] < 0 ? (nrows + 15) & ~15 : (int)a["scap"];
  RamdBuffers b = {};
  const ChainPlan p = ramd_plan_chain(&sh, &b, row0, nrows, chain_persist_wanted(&sh, &b, row0, nrows));
  int nsegs = 0;
  ChainSegment s;
  for (int r = 0; chain_segment(p, r, &s); r += s.nrows, nsegs++) printf("seg%d=%d,%d,%d,%d>%d\n", nsegs, s.row0, s.nrows, s.one, s.pad, s.early);
  printf("nsegs=%d\n", nsegs);
  return 0;
}
