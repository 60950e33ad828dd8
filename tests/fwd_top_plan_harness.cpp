// Prints whether recur_amd/csrc/fwd_top_plan.h gives a forward pass to the one-launch forward + top kernel, as key=value
// lines (tests/test_fwd_top_plan.py).  Arguments are key=value too; switches come from the environment.  Host code only.
#include <map>
#include <string>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fwd_top_plan.h"

int env_int(const char *name, int dflt) {
  const char *e = getenv(name);
  return (e && *e) ? atoi(e) : dflt;
}

int main(int argc, char **argv) {
  /* mode: RAMD_IN_* (3 text); want: RAMD_FWD_* (1 for the text top); uniform_idx < 0: staggered rings; resident, table,
   * tickets: what the residency probe found (coop_rule.h: SeatRule) */
  std::map<std::string, long long> a = {
      {"input", 42}, {"hidden", 1024}, {"output", 42}, {"streams", 256}, {"row0", 0}, {"nrows", -1}, {"mode", 3},
      {"advance", 1}, {"noise", 0}, {"fwd_only", 0}, {"want", 1}, {"rows_built", 0}, {"one_net", 0}, {"uniform_idx", 0},
      {"slab_floats", 1LL << 28}, {"bottom", 0}, {"resident", 1}, {"table", 1}, {"tickets", 0}};
  for (int i = 1; i < argc; i++) {
    const char *eq = strchr(argv[i], '=');
    std::string key(argv[i], eq ? eq - argv[i] : strlen(argv[i]));
    if (!eq || !a.count(key)) return fprintf(stderr, "unknown argument %s\n", argv[i]), 2;
    a[key] = strtoll(eq + 1, nullptr, 0);
  }
  RamdShape sh = {};
  sh.input_size = (int)a["input"], sh.hidden_size = (int)a["hidden"], sh.output_size = (int)a["output"];
  sh.I = (1 + sh.input_size + sh.hidden_size + 3) & ~3, sh.H = (sh.hidden_size + 1 + 3) & ~3, sh.O = (sh.output_size + 3) & ~3;
  sh.D = 20, sh.Scap = (int)a["streams"], sh.activation = 1;
  if (a["bottom"]) sh.b_in = (int)a["bottom"], sh.b_out = sh.input_size, sh.bI = (sh.b_in + 1 + 3) & ~3, sh.bO = (sh.b_out + 3) & ~3;
  RamdBuffers b = {};
  b.uniform_idx = (int)a["uniform_idx"], b.slab_floats = (size_t)a["slab_floats"];
  RamdFwdCall c = {};
  c.fwd_only = (int)a["fwd_only"];
  c.row0 = (int)a["row0"];
  c.nrows = a["nrows"] < 0 ? sh.Scap - c.row0 : (int)a["nrows"];
  c.mode = (int)a["mode"];
  c.ld = sh.input_size, c.global_count = c.nrows;
  c.advance = (int)a["advance"], c.noise = a["noise"] ? 0.1f : 0.0f, c.want = (int)a["want"];
  c.rows_built = (int)a["rows_built"], c.one_net = (int)a["one_net"];
  const SeatRule seats = {(int)a["resident"], (int)a["table"], (int)a["tickets"], 0, nullptr};
  const FwdPlan p = ramd_plan_forward(&sh, &b, &c);
  printf("shape_ok=%d\ntakes=%d\n", (int)fwd_top_shape_ok(&sh, &b, &c, p), (int)fwd_top_takes(&sh, &b, &c, p, seats));
  return 0;
}
