"""The training scalars a caller writes BETWEEN calls, on every weight-update path.

The library keeps the reference's ABI: callers train by writing fields of RecurNNBPTT between calls (text-predict.c sets
momentum_weight and ho_scale, charmodel-predict.c:107 cuts the prototype's learn_rate in mid-training, char_epoch.c's
schedule shrinks the noise, rnn_bptt_calculate's caller sets bptt->momentum per call).  The update is done at eight
sites, each of which takes the rates and momentum weights by a route of its own:

  1  the momentum rule in the weight-delta GEMM's epilogue (k_delta_direct, k_delta_direct_ho: whole K and K split, core
     tiles and rest rows), from set_step's pend.fuse_*
  2  ADAGRAD in the same epilogue
  3  k_apply<METHOD> fed by pending K planes (pend.slab, pend.ho_slab, e->kept), from apply_learning / apply_all
  4  k_apply<METHOD> on plain deltas (per-net calls, small nets, the bottom layer as third segment)
  5  k_fused_updates: rnn_bptt_calculate's two updates (the top layer's takes no ho_scale)
  6  the exchange step's sharded optimiser (rnn_amd_set_apply_exchange)
  7  rnn_amd_set_multi_step (set_step through its own StepSpec)
  8  the per-stream learn_rate on the device (b.lr through push_learn_rates' cache and the mailbox): the
     minimum-error-factor threshold mef / lr that decides BPTT depth

Part A (test_scalars_moved_between_calls and the subprocess cases): warm the device up with the creation values; write
a new value into the host struct and into the oracle; ONE generation on both sides from the device's state, compared at
1e-4 (replay.check: norm, largest element, element by element); move the scalar AGAIN to another value (a cache that
updates once needs the second move to show); then back to the creation value.  Part B (identity=True, and
test_all_seven_rules_element_by_element): weights, momentum and aux after the step against a float64 restatement of the
rule from the state before and the deltas the device itself stored, within a bound derived from the rule's float32
operations -- that takes the GEMM's rounding out, so it sees an update that is a fraction of a per cent off, which the
1e-4 bar on the weights cannot (one update moves a weight by ~5e-4 of the largest).

The CPU-only tests (no marker) are the guard against a vacuous case: for every (site, rule, scalar) at hidden <= 256 and
once per scalar at 1024 / 64 / 10, two ORACLES from one state, with the new and with the old value, must FAIL
replay.check against each other -- except where the rule by definition ignores the scalar, where they must PASS.
"""
import numpy as np
import pytest

import golden_cases as gc
import recur_ctypes as rc
import scalar_cases as X
import scenarios as sc

gpu = pytest.mark.gpu

# hidden 1024 / 64 streams / depth 10: the direct kernel with all of K per workgroup and the update in its epilogue, 43
# rest rows (update1); o 640: 643 float4 of W_ho per workgroup, the top layer's share not the text hook's (k_delta_direct
# rather than k_delta_direct_ho).  Hidden 512: the K split form (planes), summed by the optimiser's launch.
BIG = dict(input_size=42, hidden_size=1024, output_size=42, S=64, D=10)
BIG_WIDE = dict(BIG, output_size=640)
SPLIT = dict(input_size=42, hidden_size=512, output_size=42, S=64, D=10)
SPLIT_NOISY = dict(SPLIT, noise=0.02)
MID = dict(input_size=42, hidden_size=256, output_size=42, S=32, D=5)          # (the issue's CPU experiment's shape)
MID_NOISY = dict(MID, noise=0.05)
SMALL = dict(input_size=42, hidden_size=99, output_size=42, S=3, D=10, learn_rate=1e-3)
BOTTOM = dict(input_size=16, hidden_size=39, output_size=42, S=4, D=8, learn_rate=1e-3, bottom_inputs=42, bottom_rate_scale=0.5)
SINGLE = dict(input_size=42, hidden_size=39, output_size=42, S=1, D=8, learn_rate=1e-3)
XCHG = dict(input_size=42, hidden_size=128, output_size=42, S=32, D=6, learn_rate=1e-4)
MULTI_SMALL = dict(input_size=10, hidden_size=40, output_size=50, S=6, D=6, learn_rate=3e-3, activation=rc.RESQRT)
# BASELINE.json configs[3]'s shape class (test_gpu_callers.py's _multi_head_generation): 50 heads of 73 symbols on 1024
# hidden units, 32 streams -- the one-call step's update is then the delta GEMM's epilogue
MULTI_BIG = dict(input_size=73, hidden_size=1024, output_size=3650, S=32, D=10, learn_rate=1e-4, activation=rc.RESQRT)

ALL4 = ["ho_scale", "momentum_weight", "learn_rate", "momentum"]

# (id, site, shape, rule, scalars, rnn_bptt_calculate's batch, Part B too)
CASES = [
    # site 1: set_step -> pend.fuse_* -> the epilogue; whole K + rest rows, the top layer formed by the hook
    ("site1_weighted_1024", "char_step", BIG, rc.WEIGHTED, ALL4, 1, True),
    # site 1, wide top layer; SIMPLIFIED computes its own weight from the momentum ARGUMENT and must ignore the field
    ("site1_simplified_1024_wide_top", "char_step", BIG_WIDE, rc.SIMPLIFIED_NESTEROV, ["momentum_weight", "momentum", "ho_scale"], 1, True),
    # site 1, K split (hidden 512): the planes go to k_apply; CLASSICAL's weight is 1 whatever the field says
    ("site1_classical_512", "char_step", SPLIT, rc.CLASSICAL, ["momentum_weight", "momentum", "ho_scale"], 1, True),
    ("site1_weighted_512_noisy", "char_step", SPLIT_NOISY, rc.WEIGHTED, ["noise"] + ALL4, 1, False),
    ("site1_classical_1024", "char_step", BIG, rc.CLASSICAL, ["momentum_weight", "momentum", "ho_scale"], 1, True),
    ("site1_simplified_512", "char_step", SPLIT, rc.SIMPLIFIED_NESTEROV, ["momentum_weight", "momentum", "ho_scale"], 1, True),
    # site 2: ADAGRAD in the epilogue (pend.fuse_method 4), ballast 50
    ("site2_adagrad_1024", "char_step", BIG, rc.ADAGRAD, ["ho_scale", "learn_rate"], 1, True),
    ("site2_adagrad_512", "char_step", SPLIT, rc.ADAGRAD, ["momentum_weight", "ho_scale", "learn_rate"], 1, True),
    # site 3: NESTEROV is not the epilogue's rule: the K planes (pend.slab / pend.ho_slab) go to k_apply<1>
    ("site3_nesterov_1024_planes", "char_step", BIG, rc.NESTEROV, ["ho_scale", "learn_rate"], 1, True),
    # site 3: rnn_amd_set_calc_deltas leaves its sums as planes (e->kept), rnn_apply_learning adds them up on its way
    ("site3_kept_nesterov", "deltas_apply", MID, rc.NESTEROV, ALL4, 1, True),
    ("site3_kept_adadelta", "deltas_apply", MID, rc.ADADELTA, ALL4, 1, True),
    ("site3_kept_rprop", "deltas_apply", MID, rc.RPROP, ["ho_scale", "momentum_weight", "learn_rate"], 1, True),
    ("site3_kept_weighted_512", "deltas_apply", SPLIT, rc.WEIGHTED, ["ho_scale", "momentum_weight"], 1, True),
    # site 4: per-net calls, plain deltas (k_bptt_small's net of 99), and a bottom layer as apply_all's third segment
    ("site4_pernet_h99", "pernet", SMALL, rc.WEIGHTED, ALL4, 1, True),
    ("site4_pernet_bottom", "pernet", BOTTOM, rc.WEIGHTED, ["bottom_rate_scale", "ho_scale", "learn_rate"], 1, True),
    ("site4_batched_bottom_nesterov", "char_step", BOTTOM, rc.NESTEROV, ["bottom_rate_scale", "learn_rate", "momentum"], 1, True),
    # presynaptic_noise halved and halved again on a small set (the generator states stay exact)
    ("small_set_noisy", "char_step", MID_NOISY, rc.WEIGHTED, ["noise"], 1, False),
    # site 5: rnn_bptt_calculate; neither update takes ho_scale (the oracle decides: the guard holds it to "ignored")
    ("site5_calculate_b1", "calculate", SINGLE, rc.WEIGHTED, ALL4, 1, False),
    ("site5_calculate_b4", "calculate", SINGLE, rc.WEIGHTED, ALL4, 4, False),
    # site 7: rnn_amd_set_multi_step, the epilogue at configs[3]'s shape class and the general route on a small net
    ("site7_multi_adagrad_1024", "multi", MULTI_BIG, rc.ADAGRAD, ["ho_scale", "learn_rate"], 1, True),
    ("site7_multi_weighted_1024", "multi", MULTI_BIG, rc.WEIGHTED, ["momentum_weight", "momentum"], 1, True),
    ("site7_multi_weighted_small", "multi", MULTI_SMALL, rc.WEIGHTED, ALL4, 1, True),
    ("site7_multi_adagrad_small", "multi", MULTI_SMALL, rc.ADAGRAD, ["ho_scale", "momentum_weight", "learn_rate"], 1, True),
]

# cases that need a process of their own (the library reads its switches once): (id, environment, spec)
SUBPROCESS_CASES = [
    # site 6: the exchange step's sharded optimiser with one rank, one process, one GPU
    ("site6_exchange", {"RECUR_AMD_DIST_ONE_RANK_EXCHANGE": "1"},
     dict(exchange=True, cases=[dict(kw=XCHG, method=rc.WEIGHTED, scalars=ALL4, identity=True),
                                dict(kw=XCHG, method=rc.ADAGRAD, scalars=["ho_scale", "learn_rate"], identity=True)])),
    # site 1 behind the text step's older top launch
    ("site1_text_top2_off", {"RECUR_AMD_TEXT_TOP2": "0"},
     dict(cases=[dict(kw=BIG, method=rc.WEIGHTED, scalars=["ho_scale"], identity=True)])),
    # tools/all_fast_paths_off.env: the general kernels, one rnn_amd_set_char_step case per scalar
    ("general_kernels", None,
     dict(cases=[dict(kw=MID_NOISY, method=rc.WEIGHTED, scalars=ALL4 + ["noise"], identity=False),
                 dict(kw=BOTTOM, method=rc.WEIGHTED, scalars=["bottom_rate_scale"], identity=True)])),
]

# site 8: hot_clamps (lr 0.08: the streams' error sums meet the thresholds) after 25 generations -- found on the CPU: from
# that state the oracle's bptt_depth is (12, 12, 10, 12) with the clones' rate quartered, (12, 12, 12, 12) with it
# quadrupled and (12, 12, 11, 12) with the creation value, the prototype's rate (the update's) the same in all three
HOT_KW = dict(gc.case_kwargs(gc.TRAIN_CASES["hot_clamps"]))
HOT_WARM = 25


@pytest.fixture(scope="module")
def amd():
    lib = rc.load_amd()
    assert lib.rnn_amd_device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return lib


# ------------------------------------------------------------------------------------------------ on the device --

@gpu
@pytest.mark.parametrize("label,site,kw,method,scalars,batch,identity", CASES, ids=[c[0] for c in CASES])
def test_scalars_moved_between_calls(amd, label, site, kw, method, scalars, batch, identity):
    X.run_moves(amd, site, kw, method, scalars, batch=batch, identity=identity)


@gpu
@pytest.mark.parametrize("label,env,spec", SUBPROCESS_CASES, ids=[c[0] for c in SUBPROCESS_CASES])
def test_scalars_moved_between_calls_in_a_process_of_its_own(label, env, spec):
    res = X.run_in_subprocess(X.fast_paths_off_env() if env is None else env, spec)
    assert res["comparisons"] == 3 * sum(len(c["scalars"]) for c in spec["cases"])


def _hot_state():
    o = sc.OracleSet(**HOT_KW)
    text = X._case_text("char_step", HOT_KW)
    for i in range(HOT_WARM):
        o.char_step(text, i, rc.WEIGHTED, 0.95)
    snap = X.oracle_snapshot(o)
    o.close()
    return snap, text


def _hot_oracle_depths(snap, text):
    depths = []
    for value in X.moves("clone_rate", HOT_KW):
        o = sc.OracleSet(**HOT_KW)
        X.load_oracle(o, snap)
        X.write_scalar("clone_rate", value, None, o)
        o.char_step(text, HOT_WARM, rc.WEIGHTED, 0.95)
        depths.append(tuple(int(d) for d in o.snapshot()["bptt_depth"]))
        o.close()
    return depths


@gpu
def test_site8_the_clones_rate_on_the_device_decides_bptt_depth(amd):
    """Site 8: the per-stream learn_rate the device holds (b.lr) is the ONLY thing that differs -- every clone's rate is
    cut (then raised) and the prototype's, which is the update's, stays.  In the hot regime the threshold mef / lr ends
    a stream's BPTT loop early: from the oracle's state after 25 generations of hot_clamps the three values give three
    different depth vectors (asserted below, from the oracle), so a rate that reaches the device a call late, or not at
    all, shows in bptt_depth_sum, min_error_factor and the deltas.  Each move starts from that same state."""
    snap, text = _hot_state()
    want_depths = _hot_oracle_depths(snap, text)
    assert len(set(want_depths)) == 3, want_depths
    p = X.Pair(amd, "char_step", HOT_KW, rc.WEIGHTED)
    try:
        for n, value in enumerate(X.moves("clone_rate", HOT_KW)):
            X.load_device(amd, p.g, snap)
            p.i = HOT_WARM
            p.write("clone_rate", value)
            _, sg, so = p.one_generation("site 8 clone_rate move %d" % n)   # (bptt_depth_sum and min_error_factor in it)
            assert tuple(int(d) for d in so["bptt_depth"]) == want_depths[n]
    finally:
        p.close()


SEVEN = [rc.WEIGHTED, rc.SIMPLIFIED_NESTEROV, rc.CLASSICAL, rc.NESTEROV, rc.RPROP, rc.RPROP, rc.ADAGRAD, rc.ADADELTA]


@gpu
def test_all_seven_rules_element_by_element(amd):
    """Part B for all seven rules through rnn_apply_learning at a shape with many blocks per array: hidden 512, 50
    inputs (I = 563, not a multiple of 64) on a bottom layer of 42, aux arrays on.  Off-default scalars throughout (lr
    3e-5, ho_scale 0.7, momentum_weight 0.35, the bottom layer's scale 0.6, momentum 0.9), so an identity that holds at
    the defaults only fails.  The momentum rules run first and leave a signed momentum array, which is RPROP's previous
    gradient: both of its branches are taken, and its second step meets the zeros the first one left (RPROP twice);
    then the accumulators get their ballast for ADAGRAD and ADADELTA."""
    kw = dict(input_size=50, hidden_size=512, output_size=42, S=32, D=5, learn_rate=3e-5, seed=9, bottom_inputs=42,
              bottom_rate_scale=0.6, flags=X.AUX_FLAGS)
    g = sc.AmdBatchedSet(amd, **kw)
    text = sc.synthetic_text(30000)
    b0 = g.net.contents.bptt.contents
    b0.ho_scale, b0.momentum_weight = 0.7, 0.35
    lr = np.float32(3e-5)
    rates = {"ih": lr, "ho": lr * np.float32(0.7), "b": lr * np.float32(0.6)}
    amd.rnn_set_aux_values(g.net, 1e-4)
    for i in range(4):
        g.char_step(text, i, rc.WEIGHTED, 0.9)
    branches = set()
    for n, method in enumerate(SEVEN):
        if method == rc.ADAGRAD:
            amd.rnn_set_momentum_values(g.net, X.BALLAST)
        if method == rc.ADADELTA:
            amd.rnn_set_aux_values(g.net, 1e-3)
        before = X.device_snapshot(g)
        g.char_step_deltas(text, 4 + n)
        amd.rnn_apply_learning(g.net, method, 0.9)
        after = X.device_snapshot(g)
        assert np.abs(after["ih_delta"]).max() > 0 and np.abs(after["ho_delta"]).max() > 0 and np.abs(after["b_delta"]).max() > 0
        X.check_update_identity(before, after, method, rates, 0.9, 0.35, kw, "rule %d (call %d)" % (method, n))
        if method == rc.RPROP:
            prod = after["ih_delta"] * before["ih_m"]
            branches |= {int(s) for s in np.unique(np.sign(prod))}
    assert branches == {-1, 0, 1}, branches
    g.close()


@gpu
def test_zz_retried_generations_are_few():
    """the module's last test: how often a comparison took the next generation because of a rounding-level mask flip"""
    print("scalar cases: %(comparisons)d comparisons made, %(retried)d generations retried (%(flipped)d of %(values)d "
          "hidden values differed in being zero)" % X.COUNTS)
    assert X.COUNTS["comparisons"] > 0
    assert 1e6 * X.COUNTS["flipped"] <= 10.0 * X.COUNTS["values"], X.COUNTS
    assert 20 * X.COUNTS["retried"] <= X.COUNTS["comparisons"], X.COUNTS


# ---------------------------------------------------------------------------- the guard (CPU only: oracle vs oracle) --

def _guarded():
    seen_big = set()
    out = []
    subs = [(lab, c.get("site", "char_step"), c["kw"], c["method"], c["scalars"], 1)
            for lab, _, spec in SUBPROCESS_CASES for c in spec["cases"]]
    for label, site, kw, method, scalars, batch in [c[:6] for c in CASES] + subs:
        for scalar in scalars:
            if kw["hidden_size"] <= 256:
                out.append((label, site, kw, method, scalar, batch))
            elif kw is BIG and scalar not in seen_big:
                seen_big.add(scalar)
                out.append((label, site, kw, method, scalar, batch))
    return out


@pytest.mark.parametrize("label,site,kw,method,scalar,batch", _guarded(),
                         ids=["%s-%s" % (c[0], c[4]) for c in _guarded()])
def test_the_oracle_sees_every_move(label, site, kw, method, scalar, batch):
    """what a device with a stale scalar would look like: must fail replay.check, or pass where the rule ignores it"""
    for second in (False, True):
        diff = X.oracle_pair_differs(site, kw, method, scalar, batch, second)
        if X.rule_ignores(scalar, method, site):
            assert diff is None, "%s is ignored by rule %d by definition, yet: %s" % (scalar, method, diff)
        else:
            assert diff is not None, "moving %s (%s move) changes nothing the comparison sees" % (
                scalar, "second" if second else "first")


def test_the_oracles_bptt_depth_follows_the_clones_rate():
    snap, text = _hot_state()
    depths = _hot_oracle_depths(snap, text)
    assert len(set(depths)) == 3, depths


@pytest.mark.parametrize("method", [rc.WEIGHTED, rc.SIMPLIFIED_NESTEROV, rc.CLASSICAL, rc.NESTEROV, rc.ADAGRAD, rc.ADADELTA, rc.RPROP])
def test_the_restatement_of_the_rules_is_the_oracles(method):
    """rule() against orc_apply_learning (float32, strict build) on the oracle's own arrays with off-default scalars: within
    the derived bound -- and a rate 0.5 % off is NOT (the sharpness Part B adds to the 1e-4 bar)"""
    kw = X.full_kw(dict(input_size=16, hidden_size=39, output_size=42, S=4, D=8, learn_rate=3e-3, bottom_inputs=42,
                        bottom_rate_scale=0.6, seed=4), method)
    o = sc.OracleSet(**kw)
    text = X._case_text("char_step", kw)
    z = o.z.contents
    z.ho_scale, z.momentum_weight = 0.7, 0.35
    X.prepare_oracle(o, method)
    for i in range(6):
        o.char_step(text, i, rc.WEIGHTED if method in (rc.RPROP, rc.CLASSICAL, rc.SIMPLIFIED_NESTEROV) else method, 0.9)
    if method == rc.RPROP:   # (step sizes at the rate's level: the clamp to max_step = rate is what reads the rate)
        for k in ("ih_aux", "ho_aux", "b_aux"):
            o.arrays()[k][:] = 3e-3
    before = X.oracle_snapshot(o)
    o.char_step(text, 6, method, 0.9)
    after = X.oracle_snapshot(o)
    lr = np.float32(3e-3)
    rates = {"ih": lr, "ho": lr * np.float32(0.7), "b": lr * np.float32(0.6)}
    X.check_update_identity(before, after, method, rates, 0.9, 0.35, kw, "oracle")
    off = {k: v * np.float32(1.005) for k, v in rates.items()}
    with pytest.raises(AssertionError):
        X.check_update_identity(before, after, method, off, 0.9, 0.35, kw, "a rate 0.5 % off")
