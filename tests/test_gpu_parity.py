"""GPU parity: librecur_amd.so (HIP, gfx950) through its C ABI against

  * the committed reference vectors (tests/golden/ref_vectors.npz, produced by the
    real reference), and
  * the CPU oracle on the same seeded inputs,

at sizes the oracle finishes in seconds, plus size-independent properties at the
full BASELINE.json size (1024 hidden / 256 streams / depth 20).

Tolerance: 1e-4 relative (2-norm) on fp32 activations, gradients and weights
(BASELINE.json north_star); ring indices, generation counters and PRNG states
are bit-exact.
"""
import ctypes as C
import os

import numpy as np
import pytest

import golden_cases as gc
import recur_ctypes as rc
import replay
import scenarios as sc

pytestmark = pytest.mark.gpu
RTOL = 1e-4


@pytest.fixture(scope="module")
def amd():
    lib = rc.load_amd()
    assert lib.rnn_amd_device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return lib


@pytest.fixture(scope="module")
def orc():
    return rc.load_oracle()


# cases whose dynamics amplify rounding differences beyond 1e-4 over their length
# are compared over a prefix on the oracle instead (see test_hot_case_stepwise)
LONG_OK = [n for n in sorted(gc.TRAIN_CASES) if n not in ("hot_clamps", "bottom_hot_clamps")]


@pytest.mark.parametrize("name", LONG_OK)
def test_batched_path_matches_reference_vectors(amd, name):
    got = replay.train_api(amd, name, batched=True)
    replay.check(got, replay.golden_case(name), RTOL, exact=("index", "generation", "rng"))


@pytest.mark.parametrize("name", ["relu_weighted", "resqrt_weighted", "relu_adagrad", "single_step_h99",
                                  "depth1", "noisy", "bottom_weighted", "bottom_adagrad_noisy"])
def test_per_net_drop_in_calls_match_reference_vectors(amd, orc, name):
    got = replay.train_api(amd, name, batched=False, sbg=orc.orc_softmax_best_guess)
    replay.check(got, replay.golden_case(name), RTOL, exact=("index", "generation", "rng"))


def test_hot_case_stepwise(amd):
    """lr 0.08: ih_scale < 1 and early exits fire (recur-nn.c:387-413).  The run is
    chaotic, so every generation is checked from the oracle's own state: the GPU
    set is re-synchronised to the oracle after each step."""
    c = gc.TRAIN_CASES["hot_clamps"]
    kw = gc.case_kwargs(c)
    g = sc.AmdBatchedSet(amd, **kw)
    o = sc.OracleSet(**kw)
    _stepwise(amd, gc.case_kwargs(c), replay.text(), c["steps"], c["method"], c["D"])


def _stepwise(amd, kw, text, steps, method, depth):
    g = sc.AmdBatchedSet(amd, **kw)
    o = sc.OracleSet(**kw)
    seen_clamp = seen_exit = False
    compared = compared_clamped = skipped = 0
    for i in range(steps):
        g.char_step(text, i, method, 0.9)
        o.char_step(text, i, method, 0.9)
        sg, so = g.snapshot(), o.snapshot()
        # break decisions can legitimately flip when an error sum sits on a threshold;
        # compare only if the oracle's executed depths match the device's
        same_depth = np.allclose(sg["ih_scale"] == 1.0, so["ih_scale"] == 1.0)
        clamped = bool((so["ih_scale"] < 1.0).any())
        if same_depth:
            # 1e-4 (north_star's bar): every array here is ONE generation deep from the oracle's own state
            replay.check(sg, so, 1e-4, keys=["ih_delta", "ho_delta", "ih_w", "ho_w", "hidden", "ih_scale",
                                             "min_error_factor"], elem_floor=1e-1)  # (the hot regime's floor: replay.check)
            compared += 1
            compared_clamped += clamped
        else:
            # a stream's error sum sat on a threshold: the streams whose decision DOES agree are still held to the bar on
            # everything that is theirs alone (the deltas and weights are sums over all streams and cannot be), and the
            # disagreeing ones must be a few -- a systematic flip could not hide in the skipped half
            agree = (sg["ih_scale"] == 1.0) == (so["ih_scale"] == 1.0)
            assert agree.sum() >= len(agree) - max(1, len(agree) // 8), "break decisions differ on %d of %d streams" % (
                (~agree).sum(), len(agree))
            replay.check({k: sg[k][agree] for k in ("hidden", "ih_scale", "min_error_factor")},
                         {k: so[k][agree] for k in ("hidden", "ih_scale", "min_error_factor")}, 1e-4,
                         keys=["hidden", "ih_scale", "min_error_factor"], exact=(), elem_floor=1e-1)
            skipped += 1
        seen_clamp |= clamped
        seen_exit |= bool((so["bptt_depth"] < depth).any()) and i >= depth  # not the ring filling up
        # resynchronise the device to the oracle's state
        _load_state(amd, g, so)
    g.close()
    o.close()
    # the comparison cannot pass vacuously: both mechanisms fired, and most generations --
    # clamped ones among them -- were actually compared
    assert seen_clamp and seen_exit
    assert compared >= steps // 2 and compared_clamped >= 1, (compared, compared_clamped)
    print("stepwise: %d generations compared in full, %d on the agreeing streams only" % (compared, skipped))


@pytest.mark.parametrize("batched", [True, False])
def test_bottom_layer_in_the_hot_regime(amd, orc, batched):
    """A bottom layer under a net whose error gain gets clipped: such a stream shrinks the layer's error
    accumulator -- the ONE bottom->o_error all clones share, earlier streams and generations included -- by
    ih_scale twice (recur-nn.c:391-399) before its own bottom deltas are formed.  Neither the product nor
    the oracle did that until tools/gpu_fuzz_api.py met a clipped stream on a bottom-layer net; the oracle is
    now pinned to the reference's vectors for this regime (golden case bottom_hot_clamps, bit-exact).
    Generation by generation from a cold start, up to the first rounding-level flip of a mask or of a clip
    decision."""
    c = gc.TRAIN_CASES["bottom_hot_clamps"]
    kw = gc.case_kwargs(c)
    g = sc.AmdBatchedSet(amd, softmax_best_guess=orc.orc_softmax_best_guess, **kw)
    o = sc.OracleSet(**kw)
    t = replay.text()
    compared = clipped = 0
    for i in range(c["steps"]):
        if batched:
            g.char_step(t, i, c["method"], 0.95)
        else:
            sc.ApiSet.char_step(g, t, i, c["method"], 0.95)
        o.char_step(t, i, c["method"], 0.95)
        sg, so = g.snapshot(), o.snapshot()
        if (not np.array_equal(sg["hidden"] != 0, so["hidden"] != 0) or not np.array_equal(sg["hist"] != 0, so["hist"] != 0)
                or not np.array_equal(sg["ih_scale"] == 1.0, so["ih_scale"] == 1.0)):
            break
        # 2e-4, not 1e-4: this run is NOT re-synchronised (the bottom layer's accumulator integrates over streams and
        # generations, which is the point of the test), so every array carries the whole sequence's rounding in the hot regime
        replay.check(sg, so, 2e-4, keys=["b_delta", "b_o_error", "b_w", "b_m", "ih_delta", "ho_delta", "ih_w", "ho_w",
                                         "hidden", "ih_scale"], exact=("index", "generation"), elem_floor=1e-1)
        compared += 1
        clipped += int((so["ih_scale"] < 1.0).sum())
    assert compared >= 10 and clipped >= 3, (compared, clipped)
    g.close()
    o.close()


def test_hot_case_stepwise_on_the_dma_delta_path(amd):
    """The same regime where k_delta_dma's coefficient path matters (recur-nn.c:387-413):
    hidden 128 / 32 streams meets the LDS-DMA delta kernel's preconditions (streams % 32,
    hidden % 128), learn rate 0.08 makes ih_scale < 1 on many streams and ends chains early,
    so rows past a break (never multiplied, possibly inf) and coefficients below 1 both go
    through the staged-coefficient select."""
    kw = dict(input_size=42, hidden_size=128, output_size=42, S=32, D=8, learn_rate=0.08, seed=12)
    _stepwise(amd, kw, sc.synthetic_text(6000), 40, rc.WEIGHTED, 8)


def test_hot_case_stepwise_on_the_direct_delta_path(amd):
    """The same regime on k_delta_direct (hidden 1024: 64 x 64 tiles that own all of K, the momentum update in the
    GEMM's epilogue): at learn rate 0.08 streams are soft-clipped (coefficients below 1) and chains end early (rows past
    a break, never multiplied: coefficient 0 over whatever the step left), so the launch takes its coefficient loop --
    chosen per launch from n_exec / ih_scale -- in most generations and the all-ones loop in the others; every
    generation is compared with the oracle from the oracle's own state at 1e-4, weights included (the fused update)."""
    # (depth 10: the direct kernel wants the K loop -- depth x streams / 32 -- in whole rings of five)
    kw = dict(input_size=42, hidden_size=1024, output_size=42, S=32, D=10, learn_rate=0.08, seed=12)
    _stepwise(amd, kw, sc.synthetic_text(6000), 30, rc.WEIGHTED, 10)


@pytest.mark.parametrize("env,node", [
    ("RECUR_AMD_DELTA_DIRECT=0", "test_full_size_generation_matches_oracle"),
    ("RECUR_AMD_DELTA_DIRECT=0", "test_hot_case_stepwise_on_the_direct_delta_path"),
    # (k_delta_direct's other forms: equal shares of K for a SIMD's two waves; the top layer's delta left in the chain launch)
    ("RECUR_AMD_DELTA_FAST_PCT=0", "test_full_size_generation_matches_oracle"),
    ("RECUR_AMD_HO_IN_DELTA=0", "test_full_size_generation_matches_oracle"),
    # (the launch-per-step chain at hidden 1024, where only a switched-off one-launch chain leaves it the call:
    # k_chain_wide<16, 32> and <16, 64>; test_chain_plan.py: test_where_the_one_launch_chain_does_not_take_the_call)
    ("RECUR_AMD_CHAIN_PERSIST=0", "test_baseline_config_shapes_one_generation_matches_oracle -k per_step_wide_1024_256_3"),
    ("RECUR_AMD_CHAIN_PERSIST=0", "test_baseline_config_shapes_one_generation_matches_oracle -k per_step_wide_1024_768_3"),
])
def test_generations_with_the_direct_delta_gemm_switched_off(env, node):
    """k_delta_direct has k_delta_dma + the optimiser launch behind it (split-K planes summed by k_apply): the full-size
    generation and the hot regime at hidden 1024 once more with RECUR_AMD_DELTA_DIRECT=0, each in a process of its own
    (the library reads its switches once per process).  Likewise the one-launch chain and the launch per step behind it."""
    import os
    import subprocess
    import sys
    e = dict(os.environ, **dict(kv.split("=") for kv in env.split()))
    node, *select = node.split()
    path = "%s::%s" % (os.path.abspath(__file__), node)
    r = subprocess.run([sys.executable, "-m", "pytest", path, *select, "-q", "-x", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=e, timeout=900, cwd=os.path.dirname(os.path.abspath(__file__)))
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_the_general_kernels_alone():
    """~35 RECUR_AMD_* switches select specialised kernels, each with the general kernel it replaced
    still behind it -- and only a handful were exercised "off".  tools/all_fast_paths_off.env switches EVERY one of them off
    at once: the whole GPU suite passes on what is left (profiles/r06_all_fast_paths_off.txt: 230 of 232; the two others
    look for the one-launch chain's own give-up message).  This node runs a selection of it on every box, in a process
    of its own (the library reads its switches once): the golden replays, the fused single-net path, the sparse ranges,
    conditioning, the hot regime stepwise, a full-size generation, one shape of every sweep."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ)
    for line in open(os.path.join(here, "..", "tools", "all_fast_paths_off.env")):
        if line.strip() and not line.startswith("#"):
            k, v = line.strip().split("=")
            env[k] = v
    sel = ("golden or fused_single_net or sparse_error or conditioning or hot_case_stepwise or "
           "full_size_generation_matches_oracle or h1024_s64_d10_i42_o640 or h2048_s64 or small_set_1024_32_20 or "
           "one_sub_chain_resqrt_512 or text_step_emergency")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu",
                        "-k", sel], capture_output=True, text=True, env=env, timeout=1500, cwd=here)
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    import re
    assert int(re.search(r"(\d+) passed", r.stdout).group(1)) >= 20, r.stdout[-500:]


@pytest.mark.parametrize("act,S,lr", [(rc.RELU, 1, 0.08), (rc.RESQRT, 3, 0.05), (rc.RECLIP20, 2, 0.08),
                                      (rc.RELU, 2, 1e-3)])
def test_per_net_calls_on_a_small_net_stepwise(amd, orc, act, S, lr):
    """text-predict's default shape (99 hidden, depth 30) through the reference's per-net
    calls: rnn_bptt_calc_deltas then runs the whole of bptt_and_accumulate_error
    (recur-nn.c:303-450) as ONE workgroup (k_bptt_small).  Hot learn rates make the loop end
    early and ih_scale drop below 1 (recur-nn.c:387-413); every generation is compared from the
    oracle's own state, accumulating calls (j > 0) included."""
    kw = dict(input_size=42, hidden_size=99, output_size=42, S=S, D=30, activation=act, learn_rate=lr, seed=5)
    text = sc.synthetic_text(4000)
    g = sc.ApiSet(amd, softmax_best_guess=orc.orc_softmax_best_guess, **kw)
    o = sc.OracleSet(**kw)
    steps, compared, seen_exit, seen_clamp = 60, 0, False, False
    for i in range(steps):
        g.char_step(text, i, rc.WEIGHTED, 0.9)
        o.char_step(text, i, rc.WEIGHTED, 0.9)
        sg, so = g.snapshot(), o.snapshot()
        assert (sg["index"] == so["index"]).all() and (sg["generation"] == so["generation"]).all()
        if np.array_equal(sg["ih_scale"] == 1.0, so["ih_scale"] == 1.0):
            replay.check(sg, so, 2e-4, keys=["ih_delta", "ho_delta", "ih_w", "ho_w", "hidden", "ih_scale",
                                             "min_error_factor", "o_error"])
            compared += 1
        seen_clamp |= bool((so["ih_scale"] < 1.0).any())
        seen_exit |= bool((so["bptt_depth"] < 30).any()) and i >= 30
        _load_state(amd, g, so)
    g.close()
    o.close()
    assert compared >= steps // 2, compared
    if lr > 0.01:
        assert seen_exit and (seen_clamp or act == rc.RESQRT)


def _load_state(amd, g, snap):
    """copy an oracle snapshot into the product's host structs and declare it written"""
    n0 = g.net.contents
    b0 = n0.bptt.contents
    rc.view(n0.ih_weights, g.I, g.H)[:] = snap["ih_w"]
    rc.view(n0.ho_weights, g.H, g.O)[:] = snap["ho_w"]
    rc.view(b0.ih_momentum, g.I, g.H)[:] = snap["ih_m"]
    rc.view(b0.ho_momentum, g.H, g.O)[:] = snap["ho_m"]
    amd.rnn_amd_sync_host(g.net, rc.RNN_AMD_EVERYTHING)
    rc.view(n0.ih_weights, g.I, g.H)[:] = snap["ih_w"]
    rc.view(n0.ho_weights, g.H, g.O)[:] = snap["ho_w"]
    rc.view(b0.ih_momentum, g.I, g.H)[:] = snap["ih_m"]
    rc.view(b0.ho_momentum, g.H, g.O)[:] = snap["ho_m"]
    for j in range(g.S):
        n = g.nets[j].contents
        b = n.bptt.contents
        rc.view(b.history, g.D, g.I)[:] = snap["hist"][:, j, :]
        rc.view(n.hidden_layer, g.H)[:] = snap["hidden"][j]
        b.min_error_factor = float(snap["min_error_factor"][j])
        assert b.index == snap["index"][j]
    amd.rnn_amd_host_written(g.net, rc.RNN_AMD_EVERYTHING)


@pytest.mark.parametrize("bit,flag", replay.COND_BITS)
def test_conditioning(amd, bit, flag):
    got = replay.cond_api(amd, bit, flag)
    z = replay.golden()
    for k, v in got.items():
        want = z["cond%d.%s" % (bit, k)]
        if bit in (2, 3, 4, 6):
            assert np.array_equal(v, want), k       # pure selects / one multiply: bit-exact
        else:
            assert np.allclose(v, want, rtol=1e-6, atol=0), k


@pytest.mark.parametrize("name,batch", [("fused_b1", 1), ("fused_b4", 4)])
def test_fused_single_net_path(amd, orc, name, batch):
    got = replay.fused_api(amd, batch, orc.orc_softmax_best_guess)
    replay.check(got, replay.golden_case(name), RTOL)


@pytest.mark.parametrize("hidden,batch", [(39, 1), (39, 3), (130, 1), (130, 3)])
def test_fused_path_leaves_the_delta_arrays_as_the_reference_does(amd, orc, hidden, batch):
    """What rnn_bptt_calculate leaves in the arrays a caller can see, in a regime where ih_scale < 1: without
    batching ih_delta holds the UNSCALED sum and ih_scale goes into the rate (recur-nn.c:966-975); with batching the
    scaled sums add up and ih_delta alone is cleared after the update (977-994) -- ho_delta, left by an earlier
    rnn_bptt_calc_deltas, is not this path's to touch.  Both were found by tools/gpu_fuzz_api.py (random call
    sequences against the compiled reference); hidden 39 takes the one-workgroup BPTT, 130 the general route."""
    lib = amd
    kw = dict(input_size=30, hidden_size=hidden, output_size=30, S=4, D=6, learn_rate=0.2, seed=77)
    g = sc.AmdBatchedSet(lib, softmax_best_guess=orc.orc_softmax_best_guess, **kw)
    o = sc.OracleSet(**kw)
    t = sc.synthetic_text(2000, alphabet=30)
    for i in range(8):                                   # ordinary generations: ho_delta is now non-zero
        g.char_step(t, i, rc.WEIGHTED, 0.9)
        o.char_step(t, i, rc.WEIGHTED, 0.9)
    seen_clip = False
    c = C.c_int(0)
    for i in range(8, 8 + 7):
        lib.rnn_bptt_advance(g.net)
        g.net_error_bptt(0, int(t[i]), int(t[i + 1]))
        g.net.contents.bptt.contents.momentum = 0.9
        lib.rnn_bptt_calculate(g.net, batch)
        o.orc.orc_advance(o.z, 0)
        o.orc.orc_net_error_bptt(o.z, 0, int(t[i]), int(t[i + 1]), C.byref(c))
        o.orc.orc_bptt_calculate(o.z, 0, batch, 0.9)
        sg, so = g.snapshot(), o.snapshot()
        if not np.array_equal(sg["hidden"] != 0, so["hidden"] != 0):
            break                                        # a rounding-level mask flip ends the comparison
        seen_clip |= bool(so["ih_scale"][0] < 0.999)
        assert np.abs(so["ho_delta"]).max() > 0
        replay.check(sg, so, RTOL, keys=["ih_w", "ho_w", "ih_m", "ho_m", "ih_delta", "ho_delta", "hidden", "hist",
                                         "min_error_factor", "ih_scale"], exact=("index", "generation"),
                     elementwise=False)  # (learn rate 0.2, clipped, fifteen generations NOT re-synchronised: every array
                                         # carries the run's rounding; the element-wise bar is for one-generation-deep comparisons)
    assert seen_clip, "the regime never clipped: the test would not see a scaled ih_delta"
    g.close()
    o.close()


@pytest.mark.parametrize("hidden,S,variance,batched", [(40, 8, 0.3, True), (130, 8, 0.1, True), (256, 32, 0.1, True),
                                                       (40, 3, 0.3, False), (130, 3, 0.1, False)])
def test_reclip20_units_at_the_ceiling_are_skipped_like_zeros(amd, orc, hidden, S, variance, batched):
    """RNN_RECLIP20 with units AT the ceiling (large initial weights): bptt_and_accumulate_error skips an input row
    whose value is 20 exactly like a zero one -- no error through it and NO weight-delta row (recur-nn.c:340-341).
    The delta GEMM's history operand did not mask such rows until tools/gpu_fuzz_api.py ran into a saturated net
    (ih_delta off by several hundred per cent there).  Stepwise against the oracle, batched and per-net calls."""
    lib = amd
    # (variances at which units reach 20 within eight generations while the oracle's two builds, plain and -Ofast,
    # still agree to 1e-5: larger ones make the net chaotic)
    kw = dict(input_size=19, hidden_size=hidden, output_size=19, S=S, D=5, learn_rate=1e-5, seed=3, activation=rc.RECLIP20,
              variance=variance)
    g = sc.AmdBatchedSet(lib, softmax_best_guess=orc.orc_softmax_best_guess, **kw)
    o = sc.OracleSet(**kw)
    t = sc.synthetic_text(3000, alphabet=19)
    at_ceiling = compared = 0
    for i in range(8):
        if batched:
            g.char_step(t, i, rc.WEIGHTED, 0.9)
        else:
            sc.ApiSet.char_step(g, t, i, rc.WEIGHTED, 0.9)
        o.char_step(t, i, rc.WEIGHTED, 0.9)
        sg, so = g.snapshot(), o.snapshot()
        if any(not np.array_equal(f(sg[k]), f(so[k])) for k in ("hidden", "hist") for f in (lambda a: a != 0,
                                                                                            lambda a: a >= 20.0)):
            break                                        # a value within rounding of 0 or of 20: not a parity case
        at_ceiling += int((so["hist"] >= 20.0).sum())
        compared += 1
        replay.check(sg, so, RTOL, keys=["ih_delta", "ho_delta", "ih_w", "ho_w", "ih_m", "hidden", "hist",
                                         "min_error_factor"], exact=("index", "generation"),
                     elementwise=False)  # (a saturated net run free: the element-wise bar is for one-generation-deep comparisons)
        # ih_scale is the soft clip of a stream's summed error norms, all of which have passed through the saturated
        # net: the one value here that carries the regime's amplification (1.3e-4 at 256 / 32; the oracle's own two
        # builds differ by 2e-5 in this regime)
        replay.check(sg, so, 3 * RTOL, keys=["ih_scale"], exact=(), elementwise=False)
    assert compared >= 6 and at_ceiling > 20
    g.close()
    o.close()


def test_fused_call_after_a_regrow_keeps_the_top_layer_deltas(amd, orc):
    """rnn_bptt_calculate rewrites ih_delta only; ho_delta is whatever the last rnn_bptt_calc_deltas left.  A clone
    made in between regrows the device image (blank delta arrays on the device, the valid ones on the host): the
    fused call has to fetch them before it declares the delta arrays device-written (tools/gpu_fuzz_api.py:
    ho_delta came back as zeros)."""
    lib = amd
    kw = dict(input_size=14, hidden_size=20, output_size=14, S=5, D=6, learn_rate=1e-3, seed=9054, activation=rc.RESQRT)
    g = sc.AmdBatchedSet(lib, softmax_best_guess=orc.orc_softmax_best_guess, **kw)
    o = sc.OracleSet(**kw)
    t = sc.synthetic_text(2000, alphabet=14)
    for i in range(3):
        g.char_step(t, i, rc.WEIGHTED, 0.9)
        o.char_step(t, i, rc.WEIGHTED, 0.9)
    fl = g.net.contents.flags & ~(rc.FLAG_OWN_BPTT | rc.FLAG_OWN_WEIGHTS)
    clones = [lib.rnn_clone(g.net, fl, 5, None) for _ in range(3)]   # a fixed seed: no draw from the prototype
    rc.view(clones[2].contents.real_inputs, 14)[:] = 0
    lib.rnn_opinion(clones[2], None, 0.0)
    for cl in clones:
        lib.rnn_delete_net(cl)
    c = C.c_int(0)
    lib.rnn_bptt_advance(g.net)
    g.net_error_bptt(0, int(t[3]), int(t[4]))
    g.net.contents.bptt.contents.momentum = 0.9
    lib.rnn_bptt_calculate(g.net, 1)
    o.orc.orc_advance(o.z, 0)
    o.orc.orc_net_error_bptt(o.z, 0, int(t[3]), int(t[4]), C.byref(c))
    o.orc.orc_bptt_calculate(o.z, 0, 1, 0.9)
    sg, so = g.snapshot(), o.snapshot()
    assert np.abs(so["ho_delta"]).max() > 0
    replay.check(sg, so, RTOL, keys=["ho_delta", "ih_delta", "ih_w", "ho_w", "ih_m", "ho_m", "hidden", "hist"],
                 exact=("index", "generation"))
    g.close()
    o.close()


@pytest.mark.parametrize("hidden,S,cuts", [(20, 3, (0, 1, 3)), (48, 7, (0, 2, 5, 7)), (256, 48, (0, 4, 24, 48)),
                                           (512, 40, (0, 17, 40))])
def test_sets_over_sub_ranges_of_a_training_set(amd, orc, hidden, S, cuts):
    """A training set driven as several sets over contiguous sub-ranges of its streams (rnn_amd_set_open on
    nets + offset): row offsets that are not tile boundaries, i.e. windowed and padded launches of the one-launch
    chain for the big nets, and -- the case tools/gpu_fuzz_api.py crashed on, an integer division by zero in the
    launcher -- a net with fewer than 32 hidden units under a set that does not start at stream 0.  Against the
    oracle's per-stream loop over all the streams."""
    lib = amd
    kw = dict(input_size=21, hidden_size=hidden, output_size=21, S=S, D=4, learn_rate=1e-3 if hidden < 256 else 1e-4,
              seed=91)
    g = sc.AmdBatchedSet(lib, **kw)
    o = sc.OracleSet(**kw)
    rs = np.random.default_rng(5)
    c = C.c_int(0)
    for step in range(7):
        hot = rs.integers(0, 21, S).astype(np.int32)
        nxt = rs.integers(0, 21, S).astype(np.int32)
        for a, b in zip(cuts[:-1], cuts[1:]):
            arr = (rc.NetP * (b - a))(*[g.nets[j] for j in range(a, b)])
            h = lib.rnn_amd_set_open(arr, b - a)
            lib.rnn_amd_set_advance(h)
            lib.rnn_amd_set_one_hot_opinion(h, rc.iptr(np.ascontiguousarray(hot[a:b])), None)
            lib.rnn_amd_set_softmax_error(h, rc.iptr(np.ascontiguousarray(nxt[a:b])))
            lib.rnn_amd_set_calc_deltas(h, 1 if a else 0, None, None)
            lib.rnn_amd_set_close(h)
        lib.rnn_apply_learning(g.net, rc.WEIGHTED, 0.9)
        for j in range(S):
            o.orc.orc_advance(o.z, j)
            o.orc.orc_net_error_bptt(o.z, j, int(hot[j]), int(nxt[j]), C.byref(c))
            o.orc.orc_calc_deltas(o.z, j, 1 if j else 0, None)
        o.orc.orc_apply_learning(o.z, rc.WEIGHTED, 0.9)
    sg, so = g.snapshot(), o.snapshot()
    assert np.array_equal(sg["hidden"] != 0, so["hidden"] != 0)
    replay.check(sg, so, RTOL, keys=["ih_w", "ho_w", "ih_m", "ho_m", "ih_delta", "ho_delta", "hidden", "output", "hist",
                                     "o_error", "min_error_factor", "ih_scale"], exact=("index", "generation"))
    g.close()
    o.close()


@pytest.mark.parametrize("batched", [False, True])
def test_sparse_error_ranges(amd, batched):
    got = replay.sparse_api(amd, batched=batched)
    want = replay.golden_case("sparse")
    replay.check(got, want, RTOL, keys=["ih_w", "ho_w", "ih_m", "ho_m", "ih_delta", "ho_delta", "hidden",
                                        "output", "hist", "h_error"])


def test_error_vectors_are_rebuilt_like_the_reference(amd, orc):
    """bptt->h_error / i_error after rnn_bptt_calc_deltas (the ping-pong of
    recur-nn.c:384-386 with the zeroing of 334-337)"""
    got = replay.train_api(amd, "ragged_s7_h130", batched=False, sbg=orc.orc_softmax_best_guess)
    want = replay.golden_case("ragged_s7_h130")
    replay.check(got, want, RTOL, keys=["h_error", "i_error"])


def test_loss_statistics_match_oracle(amd):
    kw = dict(input_size=42, hidden_size=64, output_size=42, S=9, D=6, learn_rate=1e-3, seed=5)
    g = sc.AmdBatchedSet(amd, **kw)
    o = sc.OracleSet(**kw)
    text = replay.text()
    for i in range(10):
        g.char_step(text, i)
        o.char_step(text, i)
    st = g.stats()
    z = o.z.contents
    assert st.count == z.stat_count == 90 and st.correct == z.stat_correct
    assert abs(st.error - z.stat_error) < 1e-4 * abs(z.stat_error)
    assert abs(st.entropy - z.stat_entropy) < 1e-4 * abs(z.stat_entropy)
    assert abs(st.bptt_depth_sum - z.stat_depth) < 1e-9
    assert abs(st.hidden_zeros - z.stat_zeros) < 1e-3 * z.stat_zeros
    g.close()
    o.close()


def test_empty_and_edge_inputs(amd):
    # a set of one stream, depth 1, outputs narrower than a vector, all-zero inputs
    lib = amd
    net = lib.rnn_new(3, 5, 2, rc.FLAG_STANDARD, 4, None, 1, 0.01, 0.9, 0.0, rc.RELU)
    lib.rnn_randomise_weights_auto(net)
    n = net.contents
    x = np.zeros(3, np.float32)
    out = lib.rnn_opinion(net, rc.fptr(x), 0.0)
    o = rc.view(out, n.o_size).copy()
    # with all-zero real inputs and zero hidden state only the bias row acts
    w = rc.view(n.ih_weights, n.i_size, n.h_size)
    hid = np.maximum(w[0], 0)
    hid[0] = 1
    assert np.allclose(rc.view(n.hidden_layer, n.h_size), hid, rtol=1e-6)
    assert np.allclose(o, hid @ rc.view(n.ho_weights, n.h_size, n.o_size), rtol=1e-5, atol=1e-7)
    rc.view(n.bptt.contents.o_error, n.o_size)[:] = 0
    lib.rnn_bptt_calc_deltas(net, 0, None)           # zero error: zero deltas, ih_scale 1
    lib.rnn_amd_sync_host(net, rc.RNN_AMD_EVERYTHING)
    assert not rc.view(n.bptt.contents.ih_delta, n.ih_size).any()
    assert n.bptt.contents.ih_scale == 1.0 and n.generation == 1
    lib.rnn_delete_net(net)


@pytest.mark.parametrize("label,kw,steps", [
    # more BPTT steps than a wave has lanes: k_bptt_control walks the sums in chunks of 64
    ("depth70", dict(input_size=42, hidden_size=39, output_size=42, S=3, D=70, learn_rate=3e-3, seed=31), 80),
    # an output layer wider than the direct kernels take (multi-head nets): the MFMA output
    # GEMM, the stand-alone softmax and top backprop
    ("wide_output", dict(input_size=42, hidden_size=64, output_size=300, S=4, D=5, learn_rate=1e-3, seed=32), 8),
    # h_size above 2048: the extras of the chain as a GEMM, no fused text top
    ("wide_hidden", dict(input_size=42, hidden_size=2112, output_size=42, S=2, D=3, learn_rate=1e-4, seed=33), 4),
    # the LDS-DMA delta GEMM at its smallest shape (hidden 128, 32 streams) plus its rest rows,
    # and with a second generation accumulated on top (accumulate = 1 is the per-net path only,
    # so this one checks the non-accumulating batched form twice)
    ("dma_small", dict(input_size=42, hidden_size=128, output_size=42, S=32, D=6, learn_rate=1e-3, seed=34), 9),
    # the one-launch chain with 16-stream row tiles (one sub-chain per workgroup): an odd number of
    # them, a single one, and hidden 256 where four tiles share an XCD (which launches a shape gets is asserted in
    # test_chain_plan.py: test_sets_of_whole_tiles_in_one_launch has 256 / 80 / 7)
    ("chain_one_1024_48", dict(input_size=42, hidden_size=1024, output_size=42, S=48, D=6, learn_rate=1e-5, seed=35), 8),
    ("chain_one_1024_16", dict(input_size=42, hidden_size=1024, output_size=42, S=16, D=4, learn_rate=1e-5, seed=36), 6),
    ("chain_one_256_80", dict(input_size=42, hidden_size=256, output_size=42, S=80, D=7, learn_rate=1e-4, seed=37), 9),
    # sets that are not whole 16-stream tiles run the one-launch chain over the unused rows above them
    # (test_chain_plan.py: test_sets_that_are_not_whole_tiles_run_padded has 1024 / 1 / 5, 512 / 21 / 4 and 1024 / 250 / 3:
    # seven 32-stream tiles, then two 16-stream tiles of which 26 rows are real)
    ("chain_padded_256_5", dict(input_size=42, hidden_size=256, output_size=42, S=5, D=6, learn_rate=1e-4, seed=39), 9),
    ("chain_padded_1024_1", dict(input_size=42, hidden_size=1024, output_size=42, S=1, D=5, learn_rate=1e-5, seed=40), 7),
    ("chain_padded_512_21", dict(input_size=42, hidden_size=512, output_size=42, S=21, D=4, learn_rate=1e-4, seed=41), 6),
    ("chain_padded_1024_250", dict(input_size=42, hidden_size=1024, output_size=42, S=250, D=3, learn_rate=1e-5, seed=42), 4),
    # 17 tiles of 16 streams at hidden 1024: a launch of 32-stream tiles, then the last 16 streams alone
    # (test_chain_plan.py: test_more_rows_than_one_launch_seats)
    ("chain_mixed_1024_272", dict(input_size=42, hidden_size=1024, output_size=42, S=272, D=3, learn_rate=1e-5, seed=38), 4),
])
def test_fallback_and_boundary_shapes_match_oracle(amd, label, kw, steps):
    text = sc.synthetic_text(4000)
    g = sc.AmdBatchedSet(amd, **kw)
    o = sc.OracleSet(**kw)
    for i in range(steps):
        g.char_step(text, i, rc.WEIGHTED, 0.9)
        o.char_step(text, i, rc.WEIGHTED, 0.9)
    sg, so = g.snapshot(), o.snapshot()
    assert np.array_equal(sg["hidden"] != 0, so["hidden"] != 0)
    replay.check(sg, so, RTOL, keys=["ih_w", "ho_w", "ih_m", "ho_m", "ih_delta", "ho_delta", "hidden", "output",
                                     "hist", "o_error", "min_error_factor", "ih_scale"],
                 exact=("index", "generation"))
    st = g.stats()
    z = o.z.contents
    assert st.count == steps * kw["S"] and st.correct == z.stat_correct
    assert abs(st.entropy - z.stat_entropy) <= 1e-4 * abs(z.stat_entropy)
    g.close()
    o.close()


# ------------------------------------------------------------ full size --

FULL = dict(input_size=42, hidden_size=1024, output_size=42, S=256, D=20, learn_rate=1e-5, seed=1)


@pytest.fixture(scope="module")
def full_set(amd):
    g = sc.AmdBatchedSet(amd, **FULL)
    text = sc.synthetic_text(30000)
    for i in range(24):                      # the ring is full after 20
        g.char_step(text, i, rc.WEIGHTED, 0.95)
    yield g, text
    g.close()


def test_full_size_generation_matches_oracle(amd, full_set):
    """one generation at 1024 / 256 / 20 from the device's own warmed-up state"""
    g, text = full_set
    snap = g.snapshot()
    o = sc.OracleSet(**FULL)
    a = o.arrays()
    for k in ("ih_w", "ho_w", "ih_m", "ho_m", "hist", "hidden", "index", "min_error_factor"):
        a[k][:] = snap[k]
    a["generation"][:] = snap["generation"]
    g.char_step(text, 24, rc.WEIGHTED, 0.95)
    o.char_step(text, 24, rc.WEIGHTED, 0.95)
    sg, so = g.snapshot(), o.snapshot()
    assert (so["bptt_depth"] == 20).all()
    replay.check(sg, so, RTOL, keys=["ih_delta", "ho_delta", "ih_w", "ho_w", "ih_m", "ho_m", "hidden",
                                     "output", "o_error", "hist", "min_error_factor", "ih_scale"])
    o.close()


def test_mask_flips_stay_at_the_rounding_level_rate(amd, full_set):
    """The documented hazard of every fp32 comparison of this algorithm: a ReLU pre-activation within rounding
    of zero takes its mask from the summation order, and the config-size tests step over a generation in which
    that happens.  This test bounds how OFTEN it may happen, so that a kernel which got masks wrong
    systematically could not hide behind those skips: over six generations at 1024 hidden / 256 streams, each
    from the device's state, at most 10 hidden values per million may differ in zero-ness, and every one that
    does must be within 1e-5 of zero on the side where it is not zero."""
    g, text = full_set
    o = sc.OracleSet(**FULL)
    a = o.arrays()
    differing = values = 0
    for i in range(30, 36):
        snap = g.snapshot()
        for k in ("ih_w", "ho_w", "ih_m", "ho_m", "hist", "hidden", "index", "min_error_factor"):
            a[k][:] = snap[k]
        a["generation"][:] = snap["generation"]
        g.char_step(text, i, rc.WEIGHTED, 0.95)
        o.char_step(text, i, rc.WEIGHTED, 0.95)
        hg, ho = g.snapshot()["hidden"], o.snapshot()["hidden"]
        flipped = (hg != 0) != (ho != 0)
        differing += int(flipped.sum())
        values += flipped.size
        if flipped.any():
            assert np.abs(np.where(hg[flipped] != 0, hg[flipped], ho[flipped])).max() < 1e-5
    print("mask flips: %d of %d hidden values (%.2f per million)" % (differing, values, 1e6 * differing / values))
    assert 1e6 * differing / values <= 10.0
    o.close()


def test_two_hundred_generations_at_full_size_track_the_oracle(amd):
    """Long-run behaviour AT SIZE (it was pinned only at hidden 99 through the erewhon curve, and at
    full size one generation at a time from synchronised state): 200 generations of the north-star text step -- hidden
    1024, 256 streams, depth 20 -- on erewhon.txt (the synthetic symbol stream is uniform noise: nothing to learn) from
    the same cold start on the device and on the oracle, at a learn rate at which the net learns without blowing up
    (the deltas of 256 streams are summed: at 3e-6 and above the reference itself diverges within 150 generations).
    The training entropy of every window of 25 generations must track the oracle's within 1 % (the erewhon test's bar:
    200 generations amplify fp32 summation-order differences far beyond the 1e-4 of a single step), the mean executed
    BPTT depth within 1 %, and the entropy must have fallen."""
    kw = dict(input_size=42, hidden_size=1024, output_size=42, S=256, D=20, learn_rate=1e-6, seed=3)
    text = rc.encode_erewhon(amd)
    g = sc.AmdBatchedSet(amd, **kw)
    o = sc.OracleSet(fast=True, **kw)  # (the -Ofast build of the same restatement: 200 x 256 stream-steps of hidden 1024)
    g.load_text(text)
    win, n_gen = 25, 200
    ent_g, ent_o, depth_g, depth_o = [], [], [], []
    for w in range(n_gen // win):
        z = o.z.contents
        e0, c0, d0 = z.stat_entropy, z.stat_count, z.stat_depth
        for i in range(w * win, (w + 1) * win):
            g.char_step(text, i, rc.WEIGHTED, 0.9)
            o.char_step(text, i, rc.WEIGHTED, 0.9)
        st = g.stats(clear=True)
        z = o.z.contents
        ent_g.append(-st.entropy / st.count)
        depth_g.append(st.bptt_depth_sum / st.count)
        ent_o.append(-(z.stat_entropy - e0) / (z.stat_count - c0))
        depth_o.append((z.stat_depth - d0) / (z.stat_count - c0))
    print("training entropy per window  device:", np.round(ent_g, 4), " oracle:", np.round(ent_o, 4))
    assert np.allclose(ent_g, ent_o, rtol=1e-2), (ent_g, ent_o)
    assert np.allclose(depth_g, depth_o, rtol=1e-2), (depth_g, depth_o)
    assert min(ent_g[-2:]) < ent_g[0] - 0.3, ent_g  # it learns
    g.close()
    o.close()


def test_the_north_star_generation_is_reproducible_bit_for_bit(amd):
    """Every sum in the four launches of the text step has a fixed order (the weight-delta GEMM's K over eight waves in
    wave order, with fixed shares for a SIMD's two waves; the chain's K quarters; the top layer's sums by stream groups):
    two sets with the same seed, driven through the same 25 generations one after the other on the same device, must end
    with identical bits in weights, momentum, deltas, history and hidden state -- what lets ranks that hold replicas stay
    in step without ever comparing them."""
    kw = dict(input_size=42, hidden_size=1024, output_size=42, S=256, D=20, learn_rate=1e-5, seed=4)
    text = sc.synthetic_text(30000)
    snaps = []
    for _ in range(2):
        g = sc.AmdBatchedSet(amd, **kw)
        for i in range(25):
            g.char_step(text, i, rc.WEIGHTED, 0.95)
        snaps.append(g.snapshot())
        g.close()
    for k in ("ih_w", "ho_w", "ih_m", "ho_m", "ih_delta", "ho_delta", "hist", "hidden", "output", "o_error", "min_error_factor"):
        assert np.array_equal(snaps[0][k], snaps[1][k]), k


def test_a_hundred_generations_at_full_size_track_the_compiled_reference(amd):
    """The same long run against the REFERENCE ITSELF (oracle/_ref: recur-nn.c + recur-nn-init.c compiled with the
    reference's own -Ofast flags, driven through its per-net calls: rnn_bptt_advance, one-hot opinion, softmax error,
    rnn_bptt_calc_deltas per stream, one rnn_apply_learning per generation -- charmodel-predict.c:288-327), not the
    oracle's restatement of it: 100 generations at hidden 1024 / 256 streams / depth 20 on
    erewhon.txt from the same cold start; the training entropy of every window of 25 generations within 1 %.  The
    reference's entropies are recorded in tests/golden/ref_live.npz (tests/golden/make_golden_live.py)."""
    kw = gc.HUNDRED_KW
    text = rc.encode_erewhon(amd)
    ent_r = list(np.load(gc.LIVE_GOLDEN)["hundred.entropy_per_window"])
    g = sc.AmdBatchedSet(amd, **kw)
    g.load_text(text)
    win, n_gen = gc.HUNDRED_WINDOW, gc.HUNDRED_GENERATIONS
    assert len(ent_r) == n_gen // win
    ent_g = []
    for w in range(n_gen // win):
        for i in range(w * win, (w + 1) * win):
            g.char_step(text, i, rc.WEIGHTED, gc.HUNDRED_MOMENTUM)
        st = g.stats(clear=True)
        ent_g.append(-st.entropy / st.count)
    print("training entropy per window  device:", np.round(ent_g, 4), " reference:", np.round(ent_r, 4))
    assert np.allclose(ent_g, ent_r, rtol=1e-2), (ent_g, ent_r)
    assert ent_g[-1] < ent_g[0] - 0.1, ent_g  # it learns
    g.close()


@pytest.mark.parametrize("label,kw", [
    ("configs1_text_1024_64_20", dict(input_size=42, hidden_size=1024, output_size=42, S=64, D=20)),
    # a GPU's share of 256 streams over 8 GPUs (BASELINE.json configs[3]'s sharding; `bench.py --scaling strong
    # --streams-global 32`; 64 = the share over 4 GPUs is configs[1]'s shape above): two 16-stream row tiles, three
    # quarters of the chain launch's workgroups idle, the extras + control in the tails of the others
    # (test_chain_plan.py: test_sets_of_whole_tiles_in_one_launch)
    ("small_set_1024_32_20", dict(input_size=42, hidden_size=1024, output_size=42, S=32, D=20)),
    # (hidden 512: the direct weight-delta kernel with K split four ways over workgroups -- 8 x 8 tiles, 44 rest rows as
    # two pieces per workgroup -- and, 12 x 8 tiles, two ways)
    ("configs2_classify_like_512_128_30", dict(input_size=42, hidden_size=512, output_size=42, S=128, D=30)),
    ("delta_split_two_ways_512_64_10", dict(input_size=280, hidden_size=512, output_size=42, S=64, D=10)),
    ("configs4_rnnca_like_2048_512_10", dict(input_size=42, hidden_size=2048, output_size=42, S=512, D=10)),
    # hidden 2048 with fewer streams: the 64 x 64-tile chain step would leave half the chip idle (128 tiles), so
    # the step runs as 32 x 64 tiles with the K of a stage split over the wave pairs (k_chain_wide<NS, 32>);
    # 160 streams: a multiple of 32 that is not one of 64 (these two, configs4's 64 x 64 tiles above and hidden 1536
    # below: test_chain_plan.py, test_wide_nets_a_launch_per_step)
    ("wide_half_tiles_2048_256_7", dict(input_size=42, hidden_size=2048, output_size=42, S=256, D=7)),
    ("wide_half_tiles_resqrt_2048_160_4", dict(input_size=42, hidden_size=2048, output_size=42, S=160, D=4,
                                                activation=rc.RESQRT)),
    # more than 8 row tiles: the one-launch chain once per 256 streams (test_chain_plan.py: test_more_rows_than_one_launch_seats)
    ("two_chain_launches_1024_512_20", dict(input_size=42, hidden_size=1024, output_size=42, S=512, D=20)),
    # fewer than 8 row tiles: XCDs without a row tile leave at once
    ("three_row_tiles_1024_96_12", dict(input_size=42, hidden_size=1024, output_size=42, S=96, D=12)),
    # the other activations' instances of the chain kernels: one sub-chain per workgroup with the
    # RESQRT derivative (hidden 512) and the RECLIP20 row rule (hidden 256), two sub-chains with
    # RESQRT (hidden 256, 640 streams: test_chain_plan.py, test_sets_of_whole_tiles_in_one_launch), and the
    # 64 x 64-tile step with RESQRT (hidden 1536: a net the one-launch chain does not take)
    ("one_sub_chain_resqrt_512_64_8", dict(input_size=42, hidden_size=512, output_size=42, S=64, D=8,
                                           activation=rc.RESQRT)),
    ("one_sub_chain_reclip20_256_48_8", dict(input_size=42, hidden_size=256, output_size=42, S=48, D=8,
                                             activation=rc.RECLIP20)),
    ("two_sub_chains_resqrt_256_640_6", dict(input_size=42, hidden_size=256, output_size=42, S=640, D=6,
                                             activation=rc.RESQRT)),
    ("wide_step_resqrt_1536_512_4", dict(input_size=42, hidden_size=1536, output_size=42, S=512, D=4,
                                         activation=rc.RESQRT)),
    # far more streams than the north star: the one-launch chain in many launches, the delta GEMM over
    # K = S * D = 24,576 and 6,144 rows (tools/gpu_large_sets.py goes on to 16,384 streams)
    ("many_streams_256_4096_6", dict(input_size=42, hidden_size=256, output_size=42, S=4096, D=6)),
    ("many_streams_1024_1536_4", dict(input_size=42, hidden_size=1024, output_size=42, S=1536, D=4)),
    # the launch-per-step forms that nothing else selected, each at its smallest shape (test_chain_plan.py:
    # test_wide_nets_a_launch_per_step): 24 stages in 32 x 64 tiles (k_chain_wide<24, 32>: 6 x 24 = 144 tiles of 32 streams,
    # 72 of 64), and 16 stages in 32 x 64 and 64 x 64 tiles (the latter from 768 streams: 12 x 16 = 192 tiles) -- hidden
    # 1024, which the one-launch chain takes here and leaves to them in
    # test_generations_with_the_direct_delta_gemm_switched_off's process without it
    ("wide_half_step_1536_192_3", dict(input_size=42, hidden_size=1536, output_size=42, S=192, D=3)),
    ("per_step_wide_1024_256_3", dict(input_size=42, hidden_size=1024, output_size=42, S=256, D=3)),
    ("per_step_wide_1024_768_3", dict(input_size=42, hidden_size=1024, output_size=42, S=768, D=3)),
])
def test_baseline_config_shapes_one_generation_matches_oracle(amd, label, kw):
    """BASELINE.json's other configurations at their full hidden / stream / depth sizes:
    warm the ring up on the device, then one generation on both sides from the same state
    (the generic-stage chain kernel, the delta DMA kernel at other tilings, and at hidden
    2048 the dense extras GEMM and the unfused top layer)"""
    _one_generation_from_device_state(amd, kw)


def _text_step_sweep():
    """seeded: hidden sizes either side of every launcher predicate of the fused step (whole rounds of 64 x 64 tiles, the K
    split over workgroups, rest rows 0 .. 128, the top layer's share of the fused update from 11 to ~1500 float4 per
    workgroup, k_text_top2's o_size <= 64 and h_size <= 1088), streams in multiples of 32, depths that do and do not make
    whole rings of five iterations"""
    rs = np.random.default_rng(606)
    cases = []
    for hidden in (512, 768, 1024, 1536, 2048):
        for _ in range(2):
            S = 32 * int(rs.integers(1, 4))
            D = int(rs.choice([5, 8, 10, 15]))
            n_in = int(rs.choice([42, 60, 107, 150, 280]))
            n_out = int(rs.choice([42, 64, 300, 700, 1100]))
            act = int(rs.choice([rc.RELU, rc.RELU, rc.RESQRT]))
            cases.append(("h%d_s%d_d%d_i%d_o%d_a%d" % (hidden, S, D, n_in, n_out, act),
                          dict(input_size=n_in, hidden_size=hidden, output_size=n_out, S=S, D=D, activation=act)))
    # and by hand: the direct kernel's fused update (hidden 1024, whole rings of five) under wide top layers -- 643 and
    # 1105 float4 of W_ho per workgroup of 512 threads -- and its K-split form (hidden 512) under one
    for hidden, S, D, n_in, n_out in ((1024, 64, 10, 42, 640), (1024, 32, 15, 150, 1100), (512, 64, 10, 42, 1100)):
        cases.append(("h%d_s%d_d%d_i%d_o%d_wide_top" % (hidden, S, D, n_in, n_out),
                      dict(input_size=n_in, hidden_size=hidden, output_size=n_out, S=S, D=D)))
    # and tiny nets: k_text_top2's sixteen waves share h_size rows -- below 16 of them whole waves have none (the fuzzer's
    # seed 13616, round 6: their out-of-range rows of W_ho were multiplied by zero and were NaN)
    for hidden, S, D in ((7, 3, 4), (12, 1, 3), (20, 32, 5), (61, 5, 6)):
        cases.append(("h%d_s%d_d%d_tiny" % (hidden, S, D), dict(input_size=42, hidden_size=hidden, output_size=42, S=S, D=D)))
    return cases


@pytest.mark.parametrize("label,kw", _text_step_sweep())
def test_text_step_shape_sweep(amd, label, kw):
    """the fused paths update weights IN PLACE behind hand-derived launcher predicates, so a predicate that
    drifts from its kernel's assumptions trains silently wrong (round 5's missed bound on the top layer's share).  A seeded
    sweep of rnn_amd_set_char_step over shapes either side of those predicates, one generation from the device's state
    against the oracle, weights and momentum included."""
    _one_generation_from_device_state(amd, kw)


def _one_generation_from_device_state(amd, kw, prepare=None, elem_floor=1e-2):
    """(prepare: called with the device set right after it is made; elem_floor: replay.check's, for a regime whose
    measured spread in the reference itself asks for the hot regime's floor; returns the two snapshots after the compared
    generation and the number of attempts it took, for callers that go on to ask more of them)"""
    kw = dict(kw, learn_rate=1e-5, seed=3)
    g = sc.AmdBatchedSet(amd, **kw)
    if prepare:
        prepare(g)
    text = sc.synthetic_text(30000)
    n = kw["D"] + 3
    for i in range(n):
        g.char_step(text, i, rc.WEIGHTED, 0.95)
    o = sc.OracleSet(**kw)
    a = o.arrays()
    for attempt in range(4):
        # One generation on both sides from the device's state.  A pre-activation within rounding of zero may take its
        # mask from the summation order (test_mask_flips_stay_at_the_rounding_level_rate bounds how often: 10 per
        # million, each within 1e-5 of zero); a generation in which that happens is held to exactly that bound and is
        # not an element-wise parity case (the flipped unit's error exists on one side only): take the next one.
        snap = g.snapshot()
        for k in ("ih_w", "ho_w", "ih_m", "ho_m", "hist", "hidden", "index", "min_error_factor"):
            a[k][:] = snap[k]
        a["generation"][:] = snap["generation"]
        g.stats(clear=True)
        g.char_step(text, n + attempt, rc.WEIGHTED, 0.95)
        o.char_step(text, n + attempt, rc.WEIGHTED, 0.95)
        sg, so = g.snapshot(), o.snapshot()
        flipped = (sg["hidden"] != 0) != (so["hidden"] != 0)
        if not flipped.any():
            break
        assert 1e6 * flipped.sum() / flipped.size <= 10.0, "%d of %d hidden values differ in being zero" % (
            flipped.sum(), flipped.size)
        assert np.abs(np.where(sg["hidden"][flipped] != 0, sg["hidden"][flipped], so["hidden"][flipped])).max() < 1e-5
    else:
        raise AssertionError("no generation without a rounding-level mask flip in 4 attempts")
    assert g.stats().bptt_depth_sum == float(so["bptt_depth"].sum())
    replay.check(sg, so, RTOL, keys=["ih_delta", "ho_delta", "ih_w", "ho_w", "ih_m", "ho_m", "hidden",
                                     "output", "o_error", "hist", "min_error_factor", "ih_scale"], elem_floor=elem_floor)
    g.close()
    o.close()
    return sg, so, attempt + 1


def test_noise_generated_ahead_is_dropped_when_a_generator_moves(amd):
    """The set calls generate the presynaptic noise of the NEXT forward pass on a second stream
    right after the current one (noise_ahead.c).  If the caller reseeds a stream's generator
    in between (net->rng is public: recur-nn.h:158-186), the values generated ahead came from
    the old state and must not be used: every generation is compared with the oracle, generator
    states bit for bit, across such a reseeding and across a host round trip without one."""
    kw = dict(input_size=42, hidden_size=64, output_size=42, S=8, D=5, learn_rate=1e-3, seed=9, noise=0.05)
    g = sc.AmdBatchedSet(amd, **kw)
    o = sc.OracleSet(**kw)
    text = sc.synthetic_text(4000)
    for i in range(12):
        g.char_step(text, i, rc.WEIGHTED, 0.9)
        o.char_step(text, i, rc.WEIGHTED, 0.9)
        sg, so = g.snapshot(), o.snapshot()          # a host round trip: reads, changes nothing
        assert np.array_equal(sg["rng"], so["rng"]), i
        replay.check(sg, so, RTOL, keys=["hidden", "ih_w", "ho_w", "hist"], exact=("index", "generation", "rng"))
        if i in (3, 7):                               # reseed stream 2 (and 5) on both sides
            for j in ((2,) if i == 3 else (2, 5)):
                seed = 1000 + 17 * i + j
                r = g.nets[j].contents.rng
                tmp = rc.OrcRng()
                o.orc.orc_init_rand64(C.byref(tmp), seed)
                r.a, r.b, r.c, r.d = tmp.a, tmp.b, tmp.c, tmp.d
                zr = o.z.contents.rng[j]
                zr.a, zr.b, zr.c, zr.d = tmp.a, tmp.b, tmp.c, tmp.d
                amd.rnn_amd_host_written(g.nets[j], rc.RNN_AMD_STREAM)
    g.close()
    o.close()


def test_weight_noise_continues_the_generator_the_device_holds(amd, orc):
    """rnn_weight_noise (recur-nn.c:857-883) draws from net->rng.  After batched generations with
    presynaptic noise the device holds that generator (and has moved it): the noise must continue
    from THERE, twice in a row (text-predict's --periodic-weight-noise), and the next generation's
    presynaptic noise from where the weight noise stopped.  Expected values: the oracle's
    generator primitives from the state read back before the call."""
    kw = dict(input_size=12, hidden_size=24, output_size=12, S=3, D=4, learn_rate=1e-3, seed=17, noise=0.03)
    g = sc.AmdBatchedSet(amd, **kw)
    o = sc.OracleSet(**kw)
    text = sc.synthetic_text(2000) % 12
    for i in range(5):
        g.char_step(text, i, rc.WEIGHTED, 0.9)
        o.char_step(text, i, rc.WEIGHTED, 0.9)
    for rep in range(2):
        sg = g.snapshot()
        st = rc.OrcRng()
        st.a, st.b, st.c, st.d = (int(x) for x in sg["rng"][0])
        I, H, O, hs, isz, osz = g.I, g.H, g.O, 24, 12, 12
        want_ih, want_ho = sg["ih_w"].copy(), sg["ho_w"].copy()
        for y in range(hs + 1 + isz):
            for i in range(hs):
                want_ih[y, 1 + i] += np.float32(orc.orc_cheap_gaussian_noise(C.byref(st))) * np.float32(0.01)
        for y in range(hs + 1):
            for i in range(osz):
                want_ho[y, i] += np.float32(orc.orc_cheap_gaussian_noise(C.byref(st))) * np.float32(0.01)
        amd.rnn_weight_noise(g.net, 0.01)
        after = g.snapshot()
        assert np.array_equal(after["ih_w"], want_ih) and np.array_equal(after["ho_w"], want_ho), rep
        assert tuple(int(x) for x in after["rng"][0]) == (st.a, st.b, st.c, st.d)
        # the oracle follows: same weights, same generator for stream 0
        a = o.arrays()
        a["ih_w"][:] = after["ih_w"]
        a["ho_w"][:] = after["ho_w"]
        zr = o.z.contents.rng[0]
        zr.a, zr.b, zr.c, zr.d = st.a, st.b, st.c, st.d
        g.char_step(text, 5 + rep, rc.WEIGHTED, 0.9)
        o.char_step(text, 5 + rep, rc.WEIGHTED, 0.9)
        replay.check(g.snapshot(), o.snapshot(), RTOL, keys=["hidden", "ih_w", "ho_w"], exact=("index", "generation", "rng"))
    g.close()
    o.close()


@pytest.mark.parametrize("hidden,act", [(64, rc.RELU), (128, rc.RESQRT), (96, rc.RELU)])
def test_text_step_emergency_soft_clip_of_the_input_row(amd, hidden, act):
    """maybe_scale_inputs (recur-nn.c:68-81): a hidden state large enough that the input row's
    sum passes 16 * i_size; the fused assemble + forward launch (hidden 64, 128) and the
    separate kernels (hidden 96: one partial stage) must both scale the stored row and the
    sums like the reference"""
    kw = dict(input_size=42, hidden_size=hidden, output_size=42, S=32, D=4, learn_rate=1e-4, seed=5,
              activation=act)
    g = sc.AmdBatchedSet(amd, **kw)
    o = sc.OracleSet(**kw)
    text = sc.synthetic_text(4000)
    for i in range(2):
        g.char_step(text, i, rc.WEIGHTED, 0.9)
        o.char_step(text, i, rc.WEIGHTED, 0.9)
    g.sync()
    a = o.arrays()
    big = (30.0 + np.arange(g.S * g.H, dtype=np.float32).reshape(g.S, g.H) % 7).astype(np.float32)
    big[:, 0] = 1.0
    big[:, hidden + 1:] = 0.0
    for j in range(g.S):
        rc.view(g.nets[j].contents.hidden_layer, g.H)[:] = big[j]
        amd.rnn_amd_host_written(g.nets[j], rc.RNN_AMD_STREAM)
    a["hidden"][:] = big
    assert big[0].sum() + 1 > 16 * g.I          # the clip does trigger
    for i in range(2, 4):
        g.char_step(text, i, rc.WEIGHTED, 0.9)
        o.char_step(text, i, rc.WEIGHTED, 0.9)
    sg, so = g.snapshot(), o.snapshot()
    replay.check(sg, so, RTOL, keys=["hist", "hidden", "output", "o_error", "ih_delta", "ho_delta", "ih_w", "ho_w"])
    g.close()
    o.close()


def test_full_size_split_accumulation_property(amd, full_set):
    """size-independent property: the deltas of the whole set equal the deltas of
    its two halves accumulated (the reference's `j ? 1 : 0`, charmodel-predict.c:309)"""
    g, text = full_set
    lib = amd
    lib.rnn_amd_set_advance(g.handle)
    hot = np.ascontiguousarray(text[100:100 + g.S].astype(np.int32))
    tgt = np.ascontiguousarray(text[101:101 + g.S].astype(np.int32))
    lib.rnn_amd_set_one_hot_opinion(g.handle, rc.iptr(hot), None)
    lib.rnn_amd_set_softmax_error(g.handle, rc.iptr(tgt))
    lib.rnn_amd_set_calc_deltas(g.handle, 0, None, None)
    whole = g.snapshot()
    lo = np.zeros(g.S, np.uint8)
    lo[:g.S // 2] = 1
    hi = (1 - lo).astype(np.uint8)
    lib.rnn_amd_set_calc_deltas(g.handle, 0, None, rc.u8ptr(lo))
    lib.rnn_amd_set_calc_deltas(g.handle, 1, None, rc.u8ptr(hi))
    halves = g.snapshot()
    assert rc.rel_err(halves["ih_delta"], whole["ih_delta"]) < 1e-5
    assert rc.rel_err(halves["ho_delta"], whole["ho_delta"]) < 1e-5
    assert np.array_equal(halves["generation"], whole["generation"] + 1)


def test_full_size_optimiser_is_elementwise_exact(amd, full_set):
    g, text = full_set
    before = g.snapshot()
    amd.rnn_apply_learning(g.net, rc.WEIGHTED, 0.95)
    after = g.snapshot()
    lr, mw, mom = np.float32(1e-5), np.float32(0.5), np.float32(0.95)
    for w, m, d in (("ih_w", "ih_m", "ih_delta"), ("ho_w", "ho_m", "ho_delta")):
        t = before[d] * lr
        want_w = before[w] + (t + before[m] * mw)
        want_m = (before[m] + t) * mom
        assert np.allclose(after[w], want_w, rtol=1e-6, atol=1e-9)  # the device contracts to fma
        assert np.allclose(after[m], want_m, rtol=1e-6, atol=1e-9)


def test_forward_only_clone_set_matches_oracle(amd):
    """batched rnn_opinion over forward-only, weight-borrowing clones (the shape of
    rnnca's frame fill, gstrnnca.c:805-831: many cell-streams, no training)"""
    lib = amd
    n_cells, steps = 70, 5
    net = lib.rnn_new(35, 128, 3, rc.FLAG_STANDARD, 8, None, 4, 1e-3, 0.9, 0.0, rc.RELU)
    lib.rnn_randomise_weights_auto(net)
    flags = net.contents.flags & ~(rc.FLAG_OWN_BPTT | rc.FLAG_OWN_WEIGHTS)
    clones = (rc.NetP * n_cells)(*[lib.rnn_clone(net, flags, rc.SUBSEED, None) for _ in range(n_cells)])
    h = lib.rnn_amd_set_open(clones, n_cells)
    assert h
    o = sc.OracleSet(input_size=35, hidden_size=128, output_size=3, S=n_cells, D=1, seed=8,
                     shape=rc.DIST_UNIFORM, perforation=0.7)
    a = o.arrays()
    n = net.contents
    assert np.array_equal(a["ih_w"], rc.view(n.ih_weights, n.i_size, n.h_size))
    rs = np.random.default_rng(3)
    out = np.zeros((n_cells, n.o_size), np.float32)
    for _ in range(steps):
        x = rs.standard_normal((n_cells, 35)).astype(np.float32)
        lib.rnn_amd_set_opinion(h, rc.fptr(x), 35, rc.fptr(out))
        for j in range(n_cells):
            o.orc.orc_opinion(o.z, j, rc.fptr(np.ascontiguousarray(x[j])), 0.0)
        assert rc.rel_err(out, a["output"]) < RTOL
    # the per-net view of one clone agrees after a sync
    lib.rnn_amd_sync_host(clones[5], rc.RNN_AMD_STREAM)
    assert rc.rel_err(rc.view(clones[5].contents.hidden_layer, n.h_size), a["hidden"][5]) < RTOL
    # training calls on such a set are refused loudly, not silently ignored
    lib.rnn_amd_set_close(h)
    for c in clones:
        lib.rnn_delete_net(c)
    lib.rnn_delete_net(net)
    o.close()


def test_classify_shape_dense_inputs_active_mask_nesterov(amd):
    """BASELINE.json configs[2] shape (gstclassify: 512 hidden, 128 streams, dense
    features, 2 classes, Nesterov; train_channel only back-propagates the channels
    whose group was trained, gstclassify.c:2070-2130): batched calls with an active
    mask against the oracle's per-stream calls."""
    lib = amd
    S, D = 128, 12
    kw = dict(input_size=32, hidden_size=512, output_size=2, S=S, D=D, learn_rate=3e-4, seed=6)
    g = sc.AmdBatchedSet(lib, **kw)
    o = sc.OracleSet(**kw)
    a = o.arrays()
    rs = np.random.default_rng(12)
    compared = 0
    for step in range(6):
        x = (rs.standard_normal((S, 32)) * 0.5).astype(np.float32)
        err = (rs.standard_normal((S, g.O)) * 0.05).astype(np.float32)
        err[:, 2:] = 0
        active = (rs.random(S) < 0.7).astype(np.uint8)
        active[0] = 1
        # gstclassify order: opinion, error, calc_deltas, then advance
        lib.rnn_amd_set_opinion(g.handle, rc.fptr(x), 32, None)
        lib.rnn_amd_set_put_o_error(g.handle, rc.fptr(err), g.O)
        lib.rnn_bptt_clear_deltas(g.net)
        lib.rnn_amd_set_calc_deltas(g.handle, 1, None, rc.u8ptr(active))
        lib.rnn_amd_set_advance(g.handle)
        lib.rnn_apply_learning(g.net, rc.NESTEROV, 0.9)
        o.orc.orc_clear_deltas(o.z)
        for j in range(S):
            o.orc.orc_opinion(o.z, j, rc.fptr(np.ascontiguousarray(x[j])), 0.0)
            a["o_error"][j, :] = err[j]
            if active[j]:
                o.orc.orc_calc_deltas(o.z, j, 1, None)
            o.orc.orc_advance(o.z, j)
        o.orc.orc_apply_learning(o.z, rc.NESTEROV, 0.9)
        # Precondition of any fp32 comparison of this algorithm: no hidden unit sits within
        # rounding of zero -- its ReLU mask, hence its whole back-propagated error, would
        # depend on the summation order (seen: unit 505 of stream 121 was 3e-8 on the device
        # and 0 on the CPU).  Steps where that happens are not compared; every step starts
        # from the oracle's state so that they stay independent.
        sg, so = g.snapshot(), o.snapshot()
        flips = np.argwhere((sg["hidden"] != 0) != (so["hidden"] != 0))
        if len(flips) == 0:
            replay.check(sg, so, RTOL, keys=["ih_w", "ho_w", "ih_m", "ho_m", "ih_delta", "ho_delta",
                                             "hidden", "output", "hist"], exact=("index", "generation"))
            compared += 1
        _load_state(amd, g, so)
    assert compared >= 3
    g.close()
    o.close()


def test_bottom_layer_dense_inputs_clear_deltas_active_mask(amd):
    """A net on a bottom layer driven the gstclassify way (gstclassify.c:1101, 2070-2130,
    2201): dense features into the bottom layer, rnn_bptt_clear_deltas every generation
    (the only thing that ever zeroes bottom->o_error, recur-nn.c:687-692), an active
    mask, Nesterov with a bottom learn-rate scale.  Batched calls against the oracle's
    per-stream calls."""
    lib = amd
    S, D, NIN = 6, 6, 20
    kw = dict(input_size=12, hidden_size=40, output_size=3, S=S, D=D, learn_rate=3e-3, seed=21,
              bottom_inputs=NIN, bottom_rate_scale=0.25)
    g = sc.AmdBatchedSet(lib, **kw)
    o = sc.OracleSet(**kw)
    a = o.arrays()
    rs = np.random.default_rng(3)
    for step in range(10):
        x = (rs.standard_normal((S, NIN)) * 0.7).astype(np.float32)
        err = (rs.standard_normal((S, g.O)) * 0.05).astype(np.float32)
        err[:, 3:] = 0
        active = (rs.random(S) < 0.7).astype(np.uint8)
        active[0] = 1
        lib.rnn_amd_set_opinion(g.handle, rc.fptr(x), NIN, None)
        lib.rnn_amd_set_put_o_error(g.handle, rc.fptr(err), g.O)
        lib.rnn_bptt_clear_deltas(g.net)
        lib.rnn_amd_set_calc_deltas(g.handle, 1, None, rc.u8ptr(active))
        lib.rnn_amd_set_advance(g.handle)
        lib.rnn_apply_learning(g.net, rc.NESTEROV, 0.9)
        o.orc.orc_clear_deltas(o.z)
        for j in range(S):
            o.orc.orc_opinion(o.z, j, rc.fptr(np.ascontiguousarray(x[j])), 0.0)
            a["o_error"][j, :] = err[j]
            if active[j]:
                o.orc.orc_calc_deltas(o.z, j, 1, None)
            o.orc.orc_advance(o.z, j)
        o.orc.orc_apply_learning(o.z, rc.NESTEROV, 0.9)
        sg, so = g.snapshot(), o.snapshot()
        assert np.array_equal(sg["hidden"] != 0, so["hidden"] != 0)
        replay.check(sg, so, RTOL, keys=["ih_w", "ho_w", "ih_m", "ho_m", "ih_delta", "ho_delta", "hidden",
                                         "output", "hist", "b_w", "b_m", "b_delta", "b_o_error"],
                     exact=("index", "generation"))
    assert np.abs(so["b_delta"]).max() > 0 and np.abs(so["b_o_error"]).max() > 0
    g.close()
    o.close()


def test_c_driver_trains_on_erewhon():
    """tools/text_predict_amd.c (plain C against include/ + librecur_amd.so) at the
    BASELINE.json configs[1] shape: 1024 hidden, 64 streams, depth 20."""
    import os
    import re
    import subprocess
    exe = os.path.join(rc.ROOT, "build", "text_predict_amd")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.join(rc.ROOT, "recur_amd", "csrc")], check=True)
    r = subprocess.run([exe, "-f", rc.EREWHON, "-H", "1024", "-t", "64", "-d", "20", "-l", "1e-5", "-s", "300",
                        "-r", "100", "-V", "1500"], capture_output=True, text=True, timeout=600,
                       cwd=rc.ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = re.findall(r"generation\s+(\d+) t_entropy ([\d.]+) v_entropy ([\d.]+) accuracy ([\d.]+) depth ([\d.]+)\s+(\d+)/s",
                      r.stdout)
    assert [int(x[0]) for x in rows] == [100, 200, 300]
    t = [float(x[1]) for x in rows]
    v = [float(x[2]) for x in rows]
    # it learns (uniform = log2(42) = 5.39).  The validation pass of a barely trained ReLU net can
    # run away over 1500 symbols (the oracle shows the same spikes), so only the best one is checked
    assert t[-1] < t[0] and min(v) < 5.39
    assert float(rows[-1][4]) > 10                              # BPTT runs deep


def test_the_same_c_program_on_the_reference_and_on_the_product(tmp_path):
    """tools/pernet_rate.c is the reference's per-net call sequence (rnn_bptt_advance, rnn_opinion,
    the caller's softmax error, rnn_bptt_calculate / rnn_bptt_calc_deltas + rnn_apply_learning) as
    one plain C program against include/recur-nn.h.  Linked against librecur_amd.so it must print the
    mean error it printed linked against the compiled reference (oracle/_ref; recorded in
    tests/golden/ref_live.npz by tests/golden/make_golden_live.py): the drop-in boundary exercised by
    the same binary interface on both sides."""
    import os
    import re
    import subprocess
    want = list(np.load(gc.LIVE_GOLDEN)["pernet.mean_error"])
    assert len(want) == len(gc.PERNET_ARGS)
    src = os.path.join(rc.ROOT, "tools", "pernet_rate.c")
    inc = os.path.join(rc.ROOT, "include")
    lib = os.path.join(rc.ROOT, "recur_amd", "lib")
    exe_amd = str(tmp_path / "pn_amd")
    subprocess.run(["gcc", "-O2", "-std=gnu11", "-D_GNU_SOURCE", "-I" + inc, src, "-o", exe_amd, "-L" + lib,
                    "-lrecur_amd", "-Wl,-rpath," + lib, "-lm"], check=True)
    for args, ref_err in zip(gc.PERNET_ARGS, want):
        r = subprocess.run([exe_amd] + list(args), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        got = float(re.search(r"mean error ([\d.]+)", r.stdout).group(1))
        assert abs(ref_err - got) <= 1e-4 * abs(ref_err), (args, ref_err, got)


def test_text_tools_train_save_score_and_sample(tmp_path):
    """tools/text_predict_amd -> net file with the alphabet in its metadata ->
    tools/text_cross_entropy_amd and tools/text_confabulate_amd (the reference's
    text-cross-entropy.c:125-207 and text-confabulate.c:50-103 flows)."""
    import os
    import subprocess
    build = os.path.join(rc.ROOT, "build")
    subprocess.run(["make", "-s", "-C", os.path.join(rc.ROOT, "recur_amd", "csrc")], check=True)
    net = str(tmp_path / "erewhon.net")
    r = subprocess.run([os.path.join(build, "text_predict_amd"), "-f", rc.EREWHON, "-H", "99", "-t", "16", "-d", "10",
                        "-l", "1e-3", "-s", "600", "-r", "300", "-V", "1500", "-n", net],
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0 and os.path.exists(net), r.stderr[-2000:]
    excerpt = tmp_path / "excerpt.txt"
    excerpt.write_bytes(open(rc.EREWHON, "rb").read()[20000:26000])
    noise = tmp_path / "noise.txt"
    noise.write_bytes(bytes(np.random.default_rng(0).choice(list(b"zqxj;:()_"), 3000).astype(np.uint8)))
    r = subprocess.run([os.path.join(build, "text_cross_entropy_amd"), "-f", net, "-i", "10", str(excerpt), str(noise)],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    rows = dict(line.rsplit(" ", 1) for line in r.stdout.strip().splitlines())
    english, junk = float(rows[str(excerpt)]), float(rows[str(noise)])
    assert 1.0 < english < 5.0 and junk > english + 1.0        # a 600-generation net already knows English from junk
    # the same number through the library in-process (alphabet from the net's metadata)
    lib = rc.bind_char(rc.load_amd())
    n = lib.rnn_load_net(net.encode())
    a = lib.rnn_char_new_alphabet_from_net(n)
    assert a.contents.len == 42 and a.contents.flags == (rc.CHAR_CASE_INSENSITIVE | rc.CHAR_COLLAPSE_SPACE)
    raw = excerpt.read_bytes()
    ln = C.c_int(0)
    enc = lib.rnn_char_alloc_encoded_text(a, raw, len(raw), C.byref(ln), None, False)
    got = lib.rnn_char_cross_entropy(n, a, enc, ln.value, 10, None, 0)
    assert abs(got - english) < 1e-4
    lib.rnn_char_free_alphabet(a)
    lib.rnn_delete_net(n)
    # sampling: deterministic for a seed, only alphabet characters, the requested length
    runs = [subprocess.run([os.path.join(build, "text_confabulate_amd"), "-f", net, "-n", "80", "-B", "1.5", "-r", "7",
                            "-p", "the "], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
            for _ in range(2)]
    assert all(x.returncode == 0 for x in runs), runs[0].stderr[-2000:]
    out = runs[0].stdout.rstrip("\n")
    assert out == runs[1].stdout.rstrip("\n") and len(out) == 80
    assert set(out.encode()) <= set(rc.DEFAULT_CHARSET)


@pytest.mark.parametrize("leakage,noise,shape", [(0.0, 0.0, (10, 5, 40, 6, 6)), (0.35, 0.0, (10, 5, 40, 6, 6)),
                                                 (0.9, 0.02, (10, 5, 40, 6, 6)), (0.3, 0.02, (35, 56, 40, 11, 7))])
def test_multi_head_generation_matches_oracle(amd, leakage, noise, shape):
    """BASELINE.json configs[3] shape class (charmodel multi-head): the output layer is n_classes
    heads of alphabet_len symbols, each stream trains its own head and, with probability
    `leakage`, the others (charmodel-multi-predict.c:17-58), and the top layer is back-propagated
    through the per-stream error ranges that loss produces (recur-nn.c:156-196, 275-301,
    including the stale-entry behaviour of the sparse path).  The batched device step against
    the oracle's per-stream restatement; generator states bit-exact (they decide the leakage).
    The restatement of multi_softmax_error itself is not pinned by the reference (that file needs
    the generated path.h); its parts are (softmax, generator, ranged calc_deltas)."""
    lib = amd
    # the last shape: a narrow net under a very wide output layer (56 heads of 35 symbols on 40 hidden
    # units), whose top-layer delta is larger than sixteen of any other GEMM output of the net -- it
    # overran the split-K workspace until the workspace was sized for it (found by tools/gpu_stress_callers.py)
    A, NC, hidden, S, D = shape
    kw = dict(input_size=A, hidden_size=hidden, output_size=A * NC, S=S, D=D, learn_rate=3e-3 if NC < 10 else 1e-3,
              seed=41, noise=noise, activation=rc.RESQRT)
    g = sc.AmdBatchedSet(lib, **kw)
    o = sc.OracleSet(**kw)
    rs = np.random.default_rng(17)
    ranges = (C.c_int * (2 * (NC + 1)))()
    for step in range(12):
        hot = rs.integers(0, A, S).astype(np.int32)
        nxt = rs.integers(0, A, S).astype(np.int32)
        cls = rs.integers(0, NC, S).astype(np.int32)
        lib.rnn_amd_set_multi_step_deltas(g.handle, rc.iptr(hot), rc.iptr(nxt), rc.iptr(cls), A, leakage, 0)
        lib.rnn_apply_learning(g.net, rc.NESTEROV if step % 2 else rc.WEIGHTED, 0.9)
        for j in range(S):
            o.orc.orc_advance(o.z, j)
            o.orc.orc_multi_softmax_error(o.z, j, int(hot[j]), int(nxt[j]), int(cls[j]), A, leakage, ranges)
            o.orc.orc_calc_deltas(o.z, j, 1 if j else 0, ranges)
        o.orc.orc_apply_learning(o.z, rc.NESTEROV if step % 2 else rc.WEIGHTED, 0.9)
    sg, so = g.snapshot(), o.snapshot()
    assert np.array_equal(sg["hidden"] != 0, so["hidden"] != 0)
    replay.check(sg, so, RTOL, keys=["ih_w", "ho_w", "ih_m", "ho_m", "ih_delta", "ho_delta", "hidden", "output",
                                     "hist", "o_error", "min_error_factor", "ih_scale"],
                 exact=("index", "generation", "rng"))
    if leakage == 0.35:       # some, not all, foreign heads were trained in the last generation
        trained = (np.abs(so["o_error"]).reshape(S, -1)[:, :A * NC].reshape(S, NC, A).sum(axis=2) > 0).sum(axis=1)
        assert trained.min() >= 1 and trained.max() > 1 and trained.min() < NC
    g.close()
    o.close()


@pytest.mark.parametrize("combined", [False, True])
def test_class_group_loss_on_device_matches_oracle(amd, combined):
    """gstclassify's train_channel (gstclassify.c:2070-2130) with two class groups, unknown
    targets for some groups and streams, per-output error weights, Nesterov: opinion, grouped
    softmax error on the device, calc_deltas over the streams that trained something, advance,
    one update per generation after rnn_bptt_clear_deltas."""
    lib = amd
    S, D, NIN = 8, 5, 12
    goff, gsize = np.array([0, 3], np.int32), np.array([3, 4], np.int32)
    kw = dict(input_size=NIN, hidden_size=48, output_size=7, S=S, D=D, learn_rate=3e-3, seed=51)
    g = sc.AmdBatchedSet(lib, **kw)
    o = sc.OracleSet(**kw)
    rs = np.random.default_rng(23)
    weight = (0.5 + rs.random(7)).astype(np.float32)
    wins_o, wrong_o, count_o = C.c_int(0), C.c_float(0), 0
    for step in range(10):
        x = (rs.standard_normal((S, NIN)) * 0.6).astype(np.float32)
        targets = np.stack([rs.integers(-1, 3, S), rs.integers(-1, 4, S)], axis=1).astype(np.int32)
        targets[0] = (1, 2)
        targets[1] = (-1, -1)                                   # nothing to train for this stream
        trained = np.zeros(S, np.uint8)
        lib.rnn_bptt_clear_deltas(g.net)
        if combined:  # (rnn_amd_set_opinion_grouped_softmax: one call, the loss and the top backprop in one launch)
            lib.rnn_amd_set_opinion_grouped_softmax(g.handle, rc.fptr(x), NIN, 2, rc.iptr(goff), rc.iptr(gsize),
                                                    rc.iptr(targets), rc.fptr(weight) if step % 2 else None,
                                                    rc.u8ptr(trained))
        else:
            lib.rnn_amd_set_opinion(g.handle, rc.fptr(x), NIN, None)
            lib.rnn_amd_set_grouped_softmax_error(g.handle, 2, rc.iptr(goff), rc.iptr(gsize), rc.iptr(targets),
                                                  rc.fptr(weight) if step % 2 else None, rc.u8ptr(trained))
        lib.rnn_amd_set_calc_deltas(g.handle, 1, None, rc.u8ptr(trained))
        lib.rnn_amd_set_advance(g.handle)
        lib.rnn_apply_learning(g.net, rc.NESTEROV, 0.9)
        o.orc.orc_clear_deltas(o.z)
        for j in range(S):
            o.orc.orc_opinion(o.z, j, rc.fptr(np.ascontiguousarray(x[j])), 0.0)
            n = o.orc.orc_grouped_softmax_error(o.z, j, 2, rc.iptr(goff), rc.iptr(gsize),
                                                rc.iptr(np.ascontiguousarray(targets[j])),
                                                rc.fptr(weight) if step % 2 else None,
                                                C.byref(wins_o), C.byref(wrong_o))
            count_o += n
            assert bool(n) == bool(trained[j])
            if n:
                o.orc.orc_calc_deltas(o.z, j, 1, None)
            o.orc.orc_advance(o.z, j)
        o.orc.orc_apply_learning(o.z, rc.NESTEROV, 0.9)
        assert trained[0] == 1 and trained[1] == 0
    sg, so = g.snapshot(), o.snapshot()
    assert np.array_equal(sg["hidden"] != 0, so["hidden"] != 0)
    replay.check(sg, so, RTOL, keys=["ih_w", "ho_w", "ih_m", "ho_m", "ih_delta", "ho_delta", "hidden", "output",
                                     "hist", "o_error"], exact=("index", "generation"))
    st = g.stats()
    assert st.count == count_o and st.correct == wins_o.value
    assert abs(st.error - wrong_o.value) < 1e-4 * abs(wrong_o.value)
    g.close()
    o.close()


def test_mixed_call_sequences_keep_host_and_device_coherent(amd, orc):
    """One training set driven through everything a caller may interleave: batched device
    generations, the per-net drop-in calls, host-side edits of the big arrays
    (rnn_amd_sync_host / rnn_amd_host_written, text-predict.c:467), rnn_forget_history on one
    stream, a forward-only clone created after the device image exists (the engine regrows),
    cross-entropy through that clone, deleting it, and on.  Against the oracle throughout."""
    lib = rc.bind_char(amd)
    text = sc.synthetic_text(3000)
    kw = dict(input_size=42, hidden_size=48, output_size=42, S=5, D=6, learn_rate=3e-3, seed=61)
    g = sc.AmdBatchedSet(lib, softmax_best_guess=orc.orc_softmax_best_guess, **kw)
    o = sc.OracleSet(**kw)
    a = o.arrays()
    keys = ["ih_w", "ho_w", "ih_m", "ho_m", "ih_delta", "ho_delta", "hidden", "output", "hist", "o_error",
            "min_error_factor", "ih_scale"]

    def same(tag):
        sg, so = g.snapshot(), o.snapshot()
        assert np.array_equal(sg["hidden"] != 0, so["hidden"] != 0), tag
        bad = sc.compare(sg, so, RTOL, keys=keys, exact=["index", "generation"])
        assert not bad, (tag, bad)

    i = 0
    for _ in range(3):                                   # batched
        g.char_step(text, i, rc.WEIGHTED, 0.9)
        o.char_step(text, i, rc.WEIGHTED, 0.9)
        i += 1
    same("batched")
    for _ in range(2):                                   # the reference's own per-stream loop
        sc.ApiSet.char_step(g, text, i, rc.WEIGHTED, 0.9)
        o.char_step(text, i, rc.WEIGHTED, 0.9)
        i += 1
    same("per-net")
    g.char_step(text, i, rc.NESTEROV, 0.9)               # and back
    o.char_step(text, i, rc.NESTEROV, 0.9)
    i += 1
    # a host-side edit of the weights, the way text-predict boosts its diagonal
    lib.rnn_amd_sync_host(g.net, rc.RNN_AMD_WEIGHTS)
    n0 = g.net.contents
    rc.view(n0.ih_weights, g.I, g.H)[7, 9] += 0.05
    rc.view(n0.ho_weights, g.H, g.O)[3, 2] -= 0.02
    lib.rnn_amd_host_written(g.net, rc.RNN_AMD_WEIGHTS)
    a["ih_w"][7, 9] += 0.05
    a["ho_w"][3, 2] -= 0.02
    # one stream forgets its hidden state (recur-nn.c:8-16)
    lib.rnn_forget_history(g.nets[2], 0)
    a["hidden"][2, :] = 0
    a["hist"][int(a["index"][2]), 2, :kw["hidden_size"] + 1] = 0
    for _ in range(2):
        g.char_step(text, i, rc.WEIGHTED, 0.9)
        o.char_step(text, i, rc.WEIGHTED, 0.9)
        i += 1
    same("after host edits")
    # a forward-only clone made now: the device image has to grow by one row
    clone = lib.rnn_clone(g.net, n0.flags & ~(rc.FLAG_OWN_BPTT | rc.FLAG_OWN_WEIGHTS), rc.SUBSEED, None)
    seg = np.ascontiguousarray(text[500:800])
    got = lib.rnn_char_cross_entropy(clone, None, rc.u8ptr(seg), len(seg), 3, None, 0)
    v = sc.OracleSet(input_size=42, hidden_size=48, output_size=42, S=1, D=1, learn_rate=1e-3, seed=1)
    v.arrays()["ih_w"][:] = a["ih_w"]
    v.arrays()["ho_w"][:] = a["ho_w"]
    want = v.orc.orc_cross_entropy(v.z, 0, rc.u8ptr(seg), len(seg), 3)
    v.close()
    assert abs(got - want) < 1e-4 * want
    g.char_step(text, i, rc.WEIGHTED, 0.9)
    o.char_step(text, i, rc.WEIGHTED, 0.9)
    i += 1
    same("with a clone alive")
    lib.rnn_delete_net(clone)
    # the fused single-net call on the prototype in between (recur-nn.c:999-1019)
    lib.rnn_bptt_advance(g.net)
    g.net_error_bptt(0, int(text[7]), int(text[8]))
    g.net.contents.bptt.contents.momentum = 0.9
    lib.rnn_bptt_calculate(g.net, 1)
    o.orc.orc_advance(o.z, 0)
    o.orc.orc_net_error_bptt(o.z, 0, int(text[7]), int(text[8]), C.byref(C.c_int(0)))
    o.orc.orc_bptt_calculate(o.z, 0, 1, 0.9)
    same("fused single net")
    for _ in range(2):
        g.char_step(text, i, rc.WEIGHTED, 0.9)
        o.char_step(text, i, rc.WEIGHTED, 0.9)
        i += 1
    same("end")
    g.close()
    o.close()


def _random_shapes(n, seed):
    rs = np.random.default_rng(seed)
    shapes = []
    for _ in range(n):
        hidden = int(rs.choice([5, 17, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 160, 200, 256, 257]))
        shapes.append(dict(hidden=hidden, S=int(rs.choice([1, 2, 3, 7, 8, 31, 32, 33, 64])),
                           D=int(rs.choice([1, 2, 3, 5, 9])), inputs=int(rs.choice([3, 10, 42, 70])),
                           outputs=int(rs.choice([2, 5, 42, 90])),
                           act=int(rs.choice([rc.RELU, rc.RESQRT, rc.RECLIP20])),
                           method=int(rs.choice([rc.WEIGHTED, rc.NESTEROV, rc.SIMPLIFIED_NESTEROV, rc.CLASSICAL])),
                           seed=int(rs.integers(1, 1000))))
    return shapes


@pytest.mark.parametrize("shape", _random_shapes(16, 2024), ids=lambda s: "h%d_s%d_d%d_i%d_o%d_a%d" % (
    s["hidden"], s["S"], s["D"], s["inputs"], s["outputs"], s["act"]))
def test_random_shapes_match_oracle(amd, shape):
    """Tile edges: hidden sizes around the 32- and 128-wide tiles, stream counts around the 32-row
    tiles and the LDS-DMA delta GEMM's preconditions, ragged input/output widths, all activations."""
    lib = amd
    rs = np.random.default_rng(shape["seed"])
    kw = dict(input_size=shape["inputs"], hidden_size=shape["hidden"], output_size=shape["outputs"], S=shape["S"],
              D=shape["D"], learn_rate=2e-3, seed=shape["seed"], activation=shape["act"])
    g = sc.AmdBatchedSet(lib, **kw)
    o = sc.OracleSet(**kw)
    a = o.arrays()
    compared = 0
    for step in range(shape["D"] + 3):
        x = (rs.standard_normal((shape["S"], shape["inputs"])) * (rs.random((shape["S"], shape["inputs"])) < 0.6)
             ).astype(np.float32)
        err = (rs.standard_normal((shape["S"], g.O)) * 0.05).astype(np.float32)
        err[:, shape["outputs"]:] = 0
        lib.rnn_amd_set_advance(g.handle)
        lib.rnn_amd_set_opinion(g.handle, rc.fptr(x), shape["inputs"], None)
        lib.rnn_amd_set_put_o_error(g.handle, rc.fptr(err), g.O)
        lib.rnn_amd_set_calc_deltas(g.handle, 0, None, None)
        lib.rnn_apply_learning(g.net, shape["method"], 0.9)
        for j in range(shape["S"]):
            o.orc.orc_advance(o.z, j)
            o.orc.orc_opinion(o.z, j, rc.fptr(np.ascontiguousarray(x[j])), 0.0)
            a["o_error"][j, :] = err[j]
            o.orc.orc_calc_deltas(o.z, j, 1 if j else 0, None)
        o.orc.orc_apply_learning(o.z, shape["method"], 0.9)
        sg, so = g.snapshot(), o.snapshot()
        if not np.array_equal(sg["hidden"] != 0, so["hidden"] != 0):
            # a pre-activation within rounding of zero (or of 20 for RECLIP20): its mask depends on
            # the summation order; carry on from the oracle's state (see the classify-shape test)
            _load_state(amd, g, so)
            continue
        replay.check(sg, so, RTOL, keys=["ih_w", "ho_w", "ih_m", "ho_m", "ih_delta", "ho_delta", "hidden",
                                         "output", "hist", "min_error_factor", "ih_scale"],
                     exact=("index", "generation"))
        compared += 1
    g.close()
    o.close()
    assert compared >= (shape["D"] + 3 + 1) // 2, "only %d generations were compared" % compared


GIVEUP_SCRIPT = r"""
import sys
sys.path.insert(0, %(tests)r)
import recur_ctypes as rc, scenarios as sc
amd = rc.load_amd()
text = sc.synthetic_text(4000)
kw = dict(input_size=42, hidden_size=256, output_size=42, S=32, D=6, learn_rate=1e-3, seed=5)
g, o = sc.AmdBatchedSet(amd, **kw), sc.OracleSet(**kw)
for i in range(4):
    g.char_step(text, i, rc.WEIGHTED, 0.9)
    o.char_step(text, i, rc.WEIGHTED, 0.9)
bad = sc.compare(g.snapshot(), o.snapshot(), 1e-4)
print("RESULT", "ok" if not bad else "; ".join(bad))
"""


def test_a_chain_that_gives_up_in_mid_run_is_redone_a_launch_per_step():
    """A co-tenant that takes CUs in mid-run makes a one-launch chain give up.  With RECUR_AMD_CHAIN_CHECK=1 (implied by
    RECUR_AMD_CHAIN_TEST_GIVEUP=n, n > 1, which pretends that the n-th launch gave up) every chain launch is checked:
    the launcher resets the abort word, switches the kernel off for the process and runs THAT call's chain again a
    launch per step -- the results must be the oracle's, before and after (kernels_chain.hip: launch_chain_persist;
    kernels_coop.hip: coop_mark_broken)."""
    import subprocess
    import sys as _sys
    script = GIVEUP_SCRIPT.replace("for i in range(4):", "for i in range(9):")
    env = dict(os.environ, RECUR_AMD_CHAIN_TEST_GIVEUP="5")
    r = subprocess.run([_sys.executable, "-c", script % {"tests": os.path.dirname(os.path.abspath(__file__))}],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "gave up in mid-run" in r.stderr and "launch per step" in r.stderr
    assert [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1] == "RESULT ok"


def test_the_chain_beside_another_process_on_the_same_gpu():
    """round 4's default took a chain workgroup's XCD and seat from its NUMBER, which anything
    else on the GPU -- another stream of the embedding application, another process, a second GStreamer element --
    invalidates by interleaving the dispatch: the launch gave up with abort code 2 and the host process was killed.  The
    seat now comes from the CU a workgroup runs on (HW_REG_XCC_ID + HW_REG_HW_ID through the residency probe's table: coop_rule.h, k_coop.h).
    tools/gpu_cotenant_probe.py trains the north-star set while a SECOND PROCESS launches 256-workgroup kernels back to back
    (build/delta_direct_microbench: one workgroup per CU): 200 generations must go through without a give-up and a
    generation made beside the other process must match the oracle at 1e-4 -- and the same run with the workgroup-number
    map (RECUR_AMD_XCD_STATIC=1, opt-in now) must end with that abort, which is why it is no longer the default."""
    import subprocess
    import sys as _sys
    exe = os.path.join(rc.ROOT, "build", "delta_direct_microbench")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.join(rc.ROOT, "recur_amd", "csrc")], check=True)
    probe = os.path.join(rc.ROOT, "tools", "gpu_cotenant_probe.py")
    r = subprocess.run([_sys.executable, probe, "200"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    assert "running at the end of the loop" in r.stdout, r.stdout[-500:]  # (the other process WAS there)
    env = dict(os.environ, RECUR_AMD_XCD_TABLE="0", RECUR_AMD_XCD_STATIC="1")
    r = subprocess.run([_sys.executable, probe, "200"], capture_output=True, text=True, timeout=600, env=env)
    # (that run ended by abort(): its helper process dies with it -- PR_SET_PDEATHSIG in the probe -- and, belt and braces,
    # by its exact pid here: a straggler would share the GPU with whatever runs after this test)
    import re
    import signal
    m = re.search(r"other process: pid (\d+)", r.stdout)
    if m:
        try:
            os.kill(int(m.group(1)), signal.SIGKILL)
        except ProcessLookupError:
            pass
    assert r.returncode != 0 and "code 2" in r.stderr, r.stdout[-1000:] + r.stderr[-2000:]


def test_a_chain_that_gives_up_on_its_first_launch_falls_back_for_that_call():
    """The one-launch chain needs its 256 workgroups resident together; whether the device and queue grant that (no
    CU mask, no partition mode, no co-tenant holding CUs) is found out by a probe launch before the process's first
    chain (kernels_coop.hip: coop_validate).  Where the probe fails the launch-per-step chain is used from the first
    call on.  RECUR_AMD_CHAIN_TEST_GIVEUP=1 takes that branch on a healthy device: the run must say so and its
    results must be the oracle's."""
    import subprocess
    import sys as _sys
    env = dict(os.environ, RECUR_AMD_CHAIN_TEST_GIVEUP="1")
    r = subprocess.run([_sys.executable, "-c", GIVEUP_SCRIPT % {"tests": os.path.dirname(os.path.abspath(__file__))}],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "using the launch-per-step chain from here on" in r.stderr
    assert [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1] == "RESULT ok"
