// Prints what recur_amd/csrc/fwd_plan.h plans for a forward pass (ramd_launch_forward) as key=value lines
// (tests/test_fwd_plan.py).  Arguments are key=value too; switches come from the environment.  Host code only.
#include <map>
#include <string>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fwd_plan.h"

int env_int(const char *name, int dflt) {
  const char *e = getenv(name);
  return (e && *e) ? atoi(e) : dflt;
}

int main(int argc, char **argv) {
  /* mode: RAMD_IN_* (0 keep, 1 one-hot, 2 dense, 3 text); want: RAMD_FWD_* (0 whole, 1 for the text top, 2 for the dense
   * top); row0 < 0: the first training row, or the first forward-only row with fwd_only; bottom: inputs of a bottom layer */
  std::map<std::string, long long> a = {
      {"input", 42}, {"hidden", 1024}, {"output", 42}, {"streams", 256}, {"row0", -1}, {"nrows", -1}, {"mode", 3},
      {"dense", -1}, {"advance", 1}, {"noise", 0}, {"fwd_only", 0}, {"want", 0}, {"rows_built", 0}, {"one_net", 0},
      {"uniform_idx", 0}, {"slab_floats", 1LL << 28}, {"noise_spec_use", 0}, {"bottom", 0}};
  for (int i = 1; i < argc; i++) {
    const char *eq = strchr(argv[i], '=');
    std::string key(argv[i], eq ? eq - argv[i] : strlen(argv[i]));
    if (!eq || !a.count(key)) return fprintf(stderr, "unknown argument %s\n", argv[i]), 2;
    a[key] = strtoll(eq + 1, nullptr, 0);
  }
  float there; /* stands for a device array: the plan asks only whether it exists */
  RamdShape sh = {};
  sh.input_size = (int)a["input"], sh.hidden_size = (int)a["hidden"], sh.output_size = (int)a["output"];
  sh.I = (1 + sh.input_size + sh.hidden_size + 3) & ~3, sh.H = (sh.hidden_size + 1 + 3) & ~3, sh.O = (sh.output_size + 3) & ~3;
  sh.D = 20, sh.Scap = (int)a["streams"], sh.activation = 1;
  if (a["bottom"]) sh.b_in = (int)a["bottom"], sh.b_out = sh.input_size, sh.bI = (sh.b_in + 1 + 3) & ~3, sh.bO = (sh.b_out + 3) & ~3;
  RamdBuffers b = {};
  b.uniform_idx = (int)a["uniform_idx"], b.slab_floats = (size_t)a["slab_floats"], b.noise_spec_use = (int)a["noise_spec_use"];
  RamdFwdCall c = {};
  c.fwd_only = (int)a["fwd_only"];
  c.row0 = a["row0"] >= 0 ? (int)a["row0"] : c.fwd_only ? sh.Scap : 0;
  c.nrows = a["nrows"] < 0 ? sh.Scap : (int)a["nrows"];
  c.mode = (int)a["mode"];
  c.dense = (a["dense"] < 0 ? c.mode == RAMD_IN_DENSE : a["dense"] != 0) ? &there : nullptr;
  c.ld = sh.input_size, c.global_count = c.nrows;
  c.advance = (int)a["advance"], c.noise = a["noise"] ? 0.1f : 0.0f, c.want = (int)a["want"];
  c.rows_built = (int)a["rows_built"], c.one_net = (int)a["one_net"];
  const FwdPlan p = ramd_plan_forward(&sh, &b, &c);
  static const char *in[] = {"built", "bottom", "assemble", "inside"}, *hid[] = {"fused", "wide", "gemm", "small"};
  static const char *nz[] = {"none", "apply", "generate"}, *end[] = {"left", "finalize", "finalize_fused", "inside"};
  static const char *out[] = {"none", "o4", "rows", "wide", "gemm", "inside"};
  printf("I=%d\nH=%d\nO=%d\ninput=%s\nadvance_first=%d\nhidden=%s\n", sh.I, sh.H, sh.O, in[p.input], p.advance_first, hid[p.hidden]);
  printf("ns=%d\nnstages=%d\ntm=%d\ntn=%d\nblocks=%d\nuniform=%d\nnkt=%d\nks=%d\n", p.ht.ns, p.nstages, p.ht.tm, p.ht.tn, p.ht.blocks,
         p.uniform, p.nkt, p.ks);
  printf("noise=%s\nend=%s\nleft_planes=%d\nleft_partials=%d\n", nz[p.noise], end[p.end], p.left.planes, p.left.partials);
  printf("output=%s\no_ns=%d\no_tm=%d\no_tn=%d\no_blocks=%d\no_nkt=%d\no_ks=%d\n", out[p.output], p.ot.ns, p.ot.tm, p.ot.tn,
         p.ot.blocks, p.o_nkt, p.o_ks);
  return 0;
}
