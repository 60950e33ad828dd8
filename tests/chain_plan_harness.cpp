// Prints what recur_amd/csrc/chain_plan.h plans for a call of ramd_chain_steps as key=value lines
// (tests/test_chain_plan.py).  Arguments are key=value too; switches come from the environment.  Host code only.
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
  /* scap < 0: nrows rounded up to whole 16-row tiles; available: the one-launch chain's process state (probe passed, no
   * give-up), which the launcher asks only where `wanted` */
  std::map<std::string, long long> a = {{"hidden", 1024}, {"nrows", 256}, {"depth", 20}, {"row0", 0},
                                        {"scap", -1},     {"uniform_idx", 0}, {"available", 1}};
  for (int i = 1; i < argc; i++) {
    const char *eq = strchr(argv[i], '=');
    std::string key(argv[i], eq ? eq - argv[i] : strlen(argv[i]));
    if (!eq || !a.count(key)) return fprintf(stderr, "unknown argument %s\n", argv[i]), 2;
    a[key] = strtoll(eq + 1, nullptr, 0);
  }
  RamdShape sh = {};
  sh.input_size = sh.output_size = 42, sh.hidden_size = (int)a["hidden"];
  sh.I = (1 + sh.input_size + sh.hidden_size + 3) & ~3, sh.H = (sh.hidden_size + 1 + 3) & ~3, sh.O = (sh.output_size + 3) & ~3;
  sh.D = (int)a["depth"], sh.activation = 1;
  const int row0 = (int)a["row0"], nrows = (int)a["nrows"];
  sh.Scap = a["scap"] < 0 ? (nrows + 15) & ~15 : (int)a["scap"];
  RamdBuffers b = {};
  b.uniform_idx = (int)a["uniform_idx"];
  const bool wanted = chain_persist_wanted(&sh, &b, row0, nrows);
  const ChainPlan p = ramd_plan_chain(&sh, &b, row0, nrows, wanted && a["available"]);
  printf("wanted=%d\nchain_rows=%d\nwindowed=%d\n", wanted, p.chain_rows, p.windowed);
  int nsegs = 0;
  ChainSegment s;
  for (int r = 0; chain_segment(p, r, &s); r += s.nrows, nsegs++)
    printf("seg%d=%d,%d,%d,%d,%d,%d>%d,%d\n", nsegs, s.row0, s.nrows, s.one, s.pad, s.nvalid, s.vlo, s.workers, s.idle_only);
  const ChainSteps &f = p.steps;
  printf("nsegs=%d\nform=%s\nuniform=%d\nns=%d\nnstages=%d\nmt=%d\ntm=%d\ntn=%d\nblocks=%d\n", nsegs,
         f.form == CHAIN_WIDE ? "wide" : "main", f.uniform, f.ns, f.nstages, f.mt, f.tm, f.tn, f.blocks);
  /* what ramd_chain_steps returns: 0 after a one-launch chain that stood, else what the per-step form leaves */
  printf("parts=%d\nparts_stood=%d\n", f.tn_parts, nsegs ? 0 : f.tn_parts);
  return 0;
}
