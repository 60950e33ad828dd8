// Prints what recur_amd/csrc/calc_plan.h plans for a call of ramd_launch_calc_deltas as key=value lines
// (tests/test_calc_plan.py).  Arguments are key=value too; switches come from the environment.  Host code only.
#include <map>
#include <string>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "calc_plan.h"

int env_int(const char *name, int dflt) {
  const char *e = getenv(name);
  return (e && *e) ? atoi(e) : dflt;
}

int main(int argc, char **argv) {
  std::map<std::string, long long> a = {
      {"input", 42}, {"hidden", 1024}, {"output", 42}, {"streams", 256}, {"depth", 20}, {"activation", 1}, {"row0", 0},
      {"nrows", -1}, {"accumulate", 0}, {"ranges", 0}, {"range_stride", 0}, {"active", 0}, {"flags", 0}, {"uniform_idx", 0},
      {"slab_floats", 1LL << 28}, {"dense_inputs", 0}, {"mheads_alen", 0}, {"mheads_part_floats", 0}, {"ho_slab", 1},
      {"defer", 1}, {"fuse_want", 1}, {"fuse_method", 0}, {"own_slab_floats", 0}, {"half_hook", 0}, {"chain_did_ho", 0}};
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
  sh.D = (int)a["depth"], sh.Scap = (int)a["streams"], sh.activation = (int)a["activation"];
  RamdBuffers b = {};
  b.uniform_idx = (int)a["uniform_idx"], b.slab_floats = (size_t)a["slab_floats"], b.dense_inputs = (int)a["dense_inputs"];
  b.mheads_alen = (int)a["mheads_alen"], b.mheads_part_floats = (size_t)a["mheads_part_floats"];
  b.mheads_part = b.mheads_part_floats ? &there : nullptr, b.ho_slab = a["ho_slab"] ? &there : nullptr;
  RamdPendingDelta d = {};
  d.fuse_want = (int)a["fuse_want"], d.fuse_method = (int)a["fuse_method"], d.own_slab_floats = (size_t)a["own_slab_floats"];
  d.own_slab = d.own_slab_floats ? &there : nullptr;
  const int nrows = a["nrows"] < 0 ? sh.Scap : (int)a["nrows"], acc = (int)a["accumulate"], stride = (int)a["range_stride"];
  const bool ranges = a["ranges"], active = a["active"], defer = a["defer"], hook = a["half_hook"];
  const CalcPlan p = ramd_plan_calc_deltas(&sh, &b, (int)a["row0"], nrows, acc, ranges, stride, active, (unsigned)a["flags"],
                                           defer ? &d : nullptr, hook);
  static const char *top[] = {"done", "sparse", "heads", "ranged", "plain"}, *xc[] = {"none", "gather", "dense"};
  static const char *xf[] = {"control5", "control8", "control9", "dense", "gemm"};
  static const char *ho[] = {"heads", "planes", "planes_paired", "paired_summed", "summed"};
  printf("I=%d\nH=%d\nO=%d\nwriteback_first=%d\ntop=%s\ntop_nb=%d\n", sh.I, sh.H, sh.O, p.writeback_first, top[p.top], p.top_nb);
  printf("dma=%d\nhas_rest=%d\ndirect=%d\ndirect_runs=%d\ndirect_fuse=%d\n", p.dma, p.has_rest, p.direct, p.direct_runs, p.direct_fuse);
  printf("dtm=%d\ndtn=%d\ndrest=%d\nnpw=%d\ndrg=%d\ndn_it=%d\ndks=%d\nfast_its=%d\n", p.dtm, p.dtn, p.drest, p.npw, p.drg, p.dn_it,
         p.dks, p.fast_its);
  printf("ho_in_delta=%d\nho_asked=%d\nsmall=%d\n", p.ho_in_delta, p.ho_asked, p.small);
  const bool ho_done = p.ho_in_delta || (p.flags & RAMD_NO_HO_DELTA) || (p.ho_asked && a["chain_did_ho"]);
  HoGemmPlan h = {};
  if (!ho_done) h = ramd_plan_ho_gemm(&sh, &b, p, nrows, acc, ranges, stride, active, defer);
  printf("ho_gemm=%s\n", ho_done ? "none" : ho[h.form]); /* (with chain_did_ho=0: the form if the chain launch declines) */
  if (p.small) return 0;
  printf("xc_req=%s\nextras=%s\nxks=%d\nown_ws=%d\nbig=%d\nks=%d\n", xc[p.xc_req], xf[p.extras], p.xks, p.own_ws, p.big, p.ks);
  if (p.direct_runs || !p.dma) return 0;
  const bool ho_direct = p.ho_asked && a["chain_did_ho"] && !(defer && b.ho_slab);
  const DmaPlan m = ramd_plan_delta_dma(&sh, p, ranges, defer, hook, (!ho_done && h.form == HO_PAIRED_SUMMED) || ho_direct);
  printf("dma_kd=%d\ndma_blocks=%d\ndma_rest_in=%d\ndma_halves=%d\ndma_kd2=%d\ndma_blocks2=%d\ndma_ks_rest=%d\ndma_rest_off=%zu\n"
         "dma_rest_stride=%zu\n", m.kd, m.blocks, m.rest_in, m.halves, m.kd2, m.blocks2, m.ks_rest, m.rest_off, m.rest_plane);
  return 0;
}
