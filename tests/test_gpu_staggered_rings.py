"""GPU parity where the streams of a set sit at DIFFERENT positions of their BPTT rings.

Every fast path of the library asks for b->uniform_idx >= 0 -- all streams of the call at one ring position -- and the
host decides that per call from the streams' bptt->index (net_api.c: ramd_set_uniform_idx).  A caller that advances one
net of a training set on its own takes the whole set off those paths for good: k_chain_main<false> with the stages counted
at run time, calc_delta_generic with ProbDelta<false> through launch_gemm and launch_gemm2, k_assemble + the forward GEMM
with ProbFwd<false> and its un-summed planes, and input_row<false> in every kernel that reads a history row, each stream
wrapping round its ring at a step of its own.  These tests hold that family to the oracle at several row tiles, several
column tiles, a partial last K stage and a K split, with the wrap at every position, under RESQRT and RECLIP20, with a
wide top layer, heads, dense inputs under an active mask and a bottom layer (staggered_cases.CASES;
test_staggered_rings_cpu.py shows without a GPU which kernels each case gets and that its stagger would notice a wrong
row rule).  The bar is test_gpu_parity.py's: replay.check at RTOL from the device's own warmed-up state.

And the rule beside it: device_view caches the View with uniform_idx 0 and hands the real position to the kernels as an
argument, so two sets over halves of one training set, each in lock step at a position of its own, must each get theirs
in consecutive calls (test_two_halves_at_two_positions)."""
import ctypes as C
import time

import numpy as np
import pytest

import recur_ctypes as rc
import replay
import scenarios as sc
import staggered_cases as st
import test_gpu_parity as parity

pytestmark = pytest.mark.gpu
RTOL = parity.RTOL


@pytest.fixture(scope="module")
def amd():
    lib = rc.load_amd()
    assert lib.rnn_amd_device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return lib


def _positions(g):
    return [g.nets[j].contents.bptt.contents.index for j in range(g.S)]


def _assert_staggered(g, want=None):
    """the fact the host's choice rests on: the set holds min(D, S) distinct ring positions in front of the generation"""
    want = min(g.D, g.S) if want is None else want
    n = st.distinct_positions(_positions(g))
    assert n >= want, "%d distinct ring positions, %d wanted" % (n, want)


@pytest.mark.parametrize("label", st.TEXT_CASES)
def test_a_staggered_text_step_matches_the_oracle(amd, label):
    """rnn_amd_set_char_step on a staggered set: D + 3 generations on the device, then one generation on both sides from
    the device's state, ring positions included (test_gpu_parity.py: _one_generation_from_device_state, with its bound on
    rounding-level mask flips).

    reclip20_130_40_6 is compared element by element from 1e-1 of an array's largest element up, the hot regime's floor
    (replay.check), not from 1e-2: with units at the ceiling the reference's own two builds are 3.2e-4 (ih_delta), 2.2e-4
    (ho_delta) and 2.0e-4 (ih_m) apart at 1e-2 on this very shape, one generation deep from identical state, and 5.2e-5,
    2.9e-5 and 2.2e-5 at 1e-1: profiles/r08_reference_elementwise_self_difference_reclip20.txt
    (tools/ref_elementwise_self_difference.py 130,40,6,1e-5,9,5,0.1,3).  The 2-norm and largest-element bars are RTOL
    as everywhere."""
    kw = st.CASES[label]["kw"]
    t0 = time.time()
    sg, so, attempts = parity._one_generation_from_device_state(amd, kw, prepare=st.stagger_device,
                                                                elem_floor=st.CASES[label].get("elem_floor", 1e-2))
    print("%s: compared at attempt %d, %.1f s" % (label, attempts, time.time() - t0))
    # every stream has advanced as often as every other since the stagger, so the positions in front of the compared
    # generation are these turned back by one: as many distinct ones, as far apart as the stagger put them
    assert np.array_equal(sg["index"], so["index"])
    assert st.distinct_positions(sg["index"]) >= min(kw["D"], kw["S"])
    off = st.stagger_offsets(kw["S"], kw["D"])
    assert np.array_equal((sg["index"] - sg["index"][0]) % kw["D"], (off - off[0]) % kw["D"])
    if kw.get("activation") == rc.RECLIP20:
        # units AT the ceiling in the compared generation, or ProbDelta<false>'s skip of such rows was not run
        assert (so["hist"] == 20.0).any() and np.array_equal(sg["hist"] == 20.0, so["hist"] == 20.0)


@pytest.mark.parametrize("label", st.TWINS)
def test_a_staggered_set_trains_the_net_its_lock_step_twin_trains(amd, label):
    """The ring position is storage and nothing else (on the oracle bit for bit: test_staggered_rings_cpu.py), so the two
    kernel families -- one-launch chain, fused forward launch and at hidden 1024 k_delta_direct with the update in its
    epilogue, against the per-step chain, the generic GEMMs and k_apply over planes -- must train the same net: two
    device sets from the same seed on the same text, one staggered, weights and momentum at RTOL after the same number of
    generations.  The history is not compared: it is rotated.  A generation after which the two sets' hidden masks
    differ is stepped over (a pre-activation within rounding of zero), four attempts as in the helper."""
    kw = dict(st.CASES[label]["kw"], learn_rate=1e-5, seed=3)
    text = sc.synthetic_text(30000)
    a, b = sc.AmdBatchedSet(amd, **kw), sc.AmdBatchedSet(amd, **kw)
    st.stagger_device(a)
    n = kw["D"] + 3
    for i in range(n):
        a.char_step(text, i, rc.WEIGHTED, 0.95)
        b.char_step(text, i, rc.WEIGHTED, 0.95)
    for attempt in range(4):
        _assert_staggered(a)
        assert st.distinct_positions(_positions(b)) == 1
        a.char_step(text, n + attempt, rc.WEIGHTED, 0.95)
        b.char_step(text, n + attempt, rc.WEIGHTED, 0.95)
        sa, sb = a.snapshot(), b.snapshot()
        flipped = (sa["hidden"] != 0) != (sb["hidden"] != 0)
        if not flipped.any():
            break
        assert 1e6 * flipped.sum() / flipped.size <= 10.0, "%d of %d hidden values differ in being zero" % (
            flipped.sum(), flipped.size)
    else:
        raise AssertionError("no generation without a rounding-level mask flip in 4 attempts")
    print("%s twin: compared at attempt %d" % (label, attempt + 1))
    replay.check(sa, sb, RTOL, keys=["ih_w", "ho_w", "ih_m", "ho_m"], exact=("generation",))
    a.close()
    b.close()


@pytest.mark.parametrize("label", ["multi_head", "multi_head_wide"])
def test_staggered_multi_head_generation_matches_the_oracle(amd, label):
    """test_multi_head_generation_matches_oracle's (10, 5, 40, 6, 6) shape at leakage 0.35, driven the way that test
    drives it, with the stagger in front on both sides: heads of 10 symbols are per-stream ranges to the library, so the
    ranged top backprop and the top layer's own delta GEMM read staggered history rows.  And its (35, 56, 40, 11, 7) shape,
    whose heads are wide enough for the per-head kernels: the sparse top backprop and k_ho_delta_heads."""
    lib = amd
    kw = dict(st.CASES[label]["kw"], learn_rate=3e-3 if label == "multi_head" else 1e-3, seed=41, noise=0.0)
    A, NC, S = kw["input_size"], kw["output_size"] // kw["input_size"], kw["S"]
    g = sc.AmdBatchedSet(lib, **kw)
    o = sc.OracleSet(**kw)
    st.stagger_device(g)
    st.stagger_oracle(o)
    rs = np.random.default_rng(17)
    ranges = (C.c_int * (2 * (NC + 1)))()
    for step in range(12):
        hot = rs.integers(0, A, S).astype(np.int32)
        nxt = rs.integers(0, A, S).astype(np.int32)
        cls = rs.integers(0, NC, S).astype(np.int32)
        _assert_staggered(g)
        lib.rnn_amd_set_multi_step_deltas(g.handle, rc.iptr(hot), rc.iptr(nxt), rc.iptr(cls), A, 0.35, 0)
        lib.rnn_apply_learning(g.net, rc.NESTEROV if step % 2 else rc.WEIGHTED, 0.9)
        for j in range(S):
            o.orc.orc_advance(o.z, j)
            o.orc.orc_multi_softmax_error(o.z, j, int(hot[j]), int(nxt[j]), int(cls[j]), A, 0.35, ranges)
            o.orc.orc_calc_deltas(o.z, j, 1 if j else 0, ranges)
        o.orc.orc_apply_learning(o.z, rc.NESTEROV if step % 2 else rc.WEIGHTED, 0.9)
    sg, so = g.snapshot(), o.snapshot()
    assert np.array_equal(sg["hidden"] != 0, so["hidden"] != 0)
    replay.check(sg, so, RTOL, keys=["ih_w", "ho_w", "ih_m", "ho_m", "ih_delta", "ho_delta", "hidden", "output",
                                     "hist", "o_error", "min_error_factor", "ih_scale"],
                 exact=("index", "generation", "rng"))
    trained = (np.abs(so["o_error"]).reshape(S, -1)[:, :A * NC].reshape(S, NC, A).sum(axis=2) > 0).sum(axis=1)
    assert trained.min() >= 1 and trained.max() > 1 and trained.min() < NC
    g.close()
    o.close()


def test_staggered_dense_inputs_active_mask_nesterov(amd):
    """test_classify_shape_dense_inputs_active_mask_nesterov's shape with 33 streams (two row tiles of 32) and the stagger in
    front: k_extras_dense through input_row_auto, the active mask over staggered rows, the delta GEMM in its big form."""
    lib = amd
    kw = dict(st.CASES["dense_active_nesterov"]["kw"], learn_rate=3e-4, seed=6)
    S = kw["S"]
    g = sc.AmdBatchedSet(lib, **kw)
    o = sc.OracleSet(**kw)
    st.stagger_device(g)
    st.stagger_oracle(o)
    a = o.arrays()
    rs = np.random.default_rng(12)
    compared = 0
    for step in range(6):
        x = (rs.standard_normal((S, 32)) * 0.5).astype(np.float32)
        err = (rs.standard_normal((S, g.O)) * 0.05).astype(np.float32)
        err[:, 2:] = 0
        active = (rs.random(S) < 0.7).astype(np.uint8)
        active[0] = 1
        _assert_staggered(g)
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
        # (a hidden unit within rounding of zero takes its mask from the summation order: such a step is not compared, and
        # every step starts from the oracle's state -- the test this one is modelled on says why)
        sg, so = g.snapshot(), o.snapshot()
        if not ((sg["hidden"] != 0) != (so["hidden"] != 0)).any():
            replay.check(sg, so, RTOL, keys=["ih_w", "ho_w", "ih_m", "ho_m", "ih_delta", "ho_delta",
                                             "hidden", "output", "hist"], exact=("index", "generation"))
            compared += 1
        parity._load_state(amd, g, so)
    assert compared >= 3
    g.close()
    o.close()


def test_staggered_bottom_layer_dense_inputs_active_mask(amd):
    """test_bottom_layer_dense_inputs_clear_deltas_active_mask with the stagger in front: k_advance, k_bottom_forward and
    k_bottom_error / k_bottom_delta with one slot per stream."""
    lib = amd
    kw = dict(st.CASES["bottom_layer"]["kw"], learn_rate=3e-3, seed=21)
    S, NIN = kw["S"], kw["bottom_inputs"]
    g = sc.AmdBatchedSet(lib, **kw)
    o = sc.OracleSet(**kw)
    st.stagger_device(g)
    st.stagger_oracle(o)
    a = o.arrays()
    rs = np.random.default_rng(3)
    for step in range(10):
        x = (rs.standard_normal((S, NIN)) * 0.7).astype(np.float32)
        err = (rs.standard_normal((S, g.O)) * 0.05).astype(np.float32)
        err[:, 3:] = 0
        active = (rs.random(S) < 0.7).astype(np.uint8)
        active[0] = 1
        _assert_staggered(g)
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


def test_two_halves_at_two_positions(amd):
    """Hidden 256 / 64 streams / depth 6, streams 32..63 two ring positions ahead of streams 0..31.  Seven generations
    driven as two sets over [0, 32) and [32, 64) (rnn_amd_set_open on nets + offset, the second accumulating on the first,
    one rnn_apply_learning): each call is in lock step at ITS position, so the one-launch chain runs with 32 rows each
    and must be handed this call's position, not the one cached with the View.  Then two generations as one set over all
    64 rows -- staggered: the set crosses to the other family of kernels.  Against the oracle's per-stream loop."""
    lib = amd
    S, D = 64, 6
    kw = dict(input_size=42, hidden_size=256, output_size=42, S=S, D=D, learn_rate=1e-4, seed=91)
    g = sc.AmdBatchedSet(lib, **kw)
    o = sc.OracleSet(**kw)
    for j in range(32, 64):
        for _ in range(2):
            lib.rnn_bptt_advance(g.nets[j])
            o.orc.orc_advance(o.z, j)
    rs = np.random.default_rng(5)
    c = C.c_int(0)
    keys = ["ih_w", "ho_w", "ih_m", "ho_m", "ih_delta", "ho_delta", "hidden", "output", "hist", "o_error",
            "min_error_factor", "ih_scale"]

    def oracle_generation(hot, nxt):
        for j in range(S):
            o.orc.orc_advance(o.z, j)
            o.orc.orc_net_error_bptt(o.z, j, int(hot[j]), int(nxt[j]), C.byref(c))
            o.orc.orc_calc_deltas(o.z, j, 1 if j else 0, None)
        o.orc.orc_apply_learning(o.z, rc.WEIGHTED, 0.9)

    def same():
        sg, so = g.snapshot(), o.snapshot()
        assert np.array_equal(sg["hidden"] != 0, so["hidden"] != 0)
        replay.check(sg, so, RTOL, keys=keys, exact=("index", "generation"))

    for step in range(7):
        hot = rs.integers(0, 42, S).astype(np.int32)
        nxt = rs.integers(0, 42, S).astype(np.int32)
        pos = _positions(g)
        assert len(set(pos[:32])) == 1 and len(set(pos[32:])) == 1 and (pos[32] - pos[0]) % D == 2
        for lo, hi in ((0, 32), (32, 64)):
            arr = (rc.NetP * (hi - lo))(*[g.nets[j] for j in range(lo, hi)])
            h = lib.rnn_amd_set_open(arr, hi - lo)
            lib.rnn_amd_set_advance(h)
            lib.rnn_amd_set_one_hot_opinion(h, rc.iptr(np.ascontiguousarray(hot[lo:hi])), None)
            lib.rnn_amd_set_softmax_error(h, rc.iptr(np.ascontiguousarray(nxt[lo:hi])))
            lib.rnn_amd_set_calc_deltas(h, 1 if lo else 0, None, None)
            lib.rnn_amd_set_close(h)
        lib.rnn_apply_learning(g.net, rc.WEIGHTED, 0.9)
        oracle_generation(hot, nxt)
    same()
    for step in range(2):
        hot = rs.integers(0, 42, S).astype(np.int32)
        nxt = rs.integers(0, 42, S).astype(np.int32)
        _assert_staggered(g, want=2)
        lib.rnn_amd_set_advance(g.handle)
        lib.rnn_amd_set_one_hot_opinion(g.handle, rc.iptr(hot), None)
        lib.rnn_amd_set_softmax_error(g.handle, rc.iptr(nxt))
        lib.rnn_amd_set_calc_deltas(g.handle, 0, None, None)
        lib.rnn_apply_learning(g.net, rc.WEIGHTED, 0.9)
        oracle_generation(hot, nxt)
    same()
    g.close()
    o.close()
