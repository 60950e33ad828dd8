"""Parrot's trainer on the device (gstparrot.c: train_net 464-477, maybe_learn 487-554): rnn_amd_set_tanh_error
(k_dense_loss_row<TanhLossRule>), rnn_amd_set_opinion_tanh_error (k_text_top<3>), rnn_amd_set_dense_step_tanh and
rnn_amd_set_dense_steps_tanh, and tools/parrot_train_amd.

  1. the separate kernel against the numpy rule (tests/parrot_cases.py) on the fetched raw answers, bit for bit, and on a
     written net whose rows hold the tanh's clamp, its neighbours, infinities and NaN;
  2. one generation from the device's state against the oracle twin, at the project's parity bar, through each of the
     three call forms, at every wave boundary of the one-launch loss and past it; the set's statistics against the float64
     sum of the oracle's terms;
  3. a saturated net: answers exactly +-1, error and deltas exactly 0;
  4. the one-launch form against the separate calls over six generations, with and without an intruder between loss and
     delta call, and the deferred top backprop's flag;
  5. the many-step call against a loop of single steps, bit for bit, chained blocks and conditioning included;
  6. exact_cases' zero-answer net: tanh(0) is 0, the error is the target, and the generation equals the oracle's in every
     element, and the compiled reference's (a test of its own, skipped visibly where the reference is not built);
  7. tools/parrot_train_amd learns the CPU half's designed signal and tools/parrot_dream_amd plays the saved net.
tests/test_parrot_cases_cpu.py shows on the oracle alone that these cases can notice a failure."""
import os
import subprocess

import numpy as np
import pytest

import exact_cases as ec
import loss_edge_cases as le
import parrot_cases as pc
import recur_ctypes as rc
import replay
import scenarios as sc
from recur_amd.drivers import train_frames
from test_gpu_callers import _same_mask, _sync_oracle_to

pytestmark = pytest.mark.gpu
F = np.float32
RTOL = 1e-4
M = pc.MOMENTUM
TOP_DONE = 16  # RNN_AMD_DEFERRED_TOP_DONE


@pytest.fixture(scope="module")
def amd():
    lib = rc.load_amd()
    assert lib.rnn_amd_device_count() >= 1, "no HIP device: the product has no CPU fallback"
    rc.bind_char(lib)
    return lib


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


def write_top_layer(lib, g, ho):
    lib.rnn_amd_sync_host(g.net, rc.RNN_AMD_EVERYTHING)
    rc.view(g.net.contents.ho_weights, g.H, g.O)[:] = ho
    lib.rnn_amd_host_written(g.net, rc.RNN_AMD_WEIGHTS)


def generation(lib, g, form, x, t, n, planted=None):
    """one generation of parrot's trainer through one of the three call forms"""
    x, t = np.ascontiguousarray(x, F), np.ascontiguousarray(t, F)
    if planted is not None:
        e = pc.padded_error(planted, g.O)
        lib.rnn_amd_set_put_o_error(g.handle, rc.fptr(e), g.O)
    if form == "dense_step":
        lib.rnn_amd_set_dense_step_tanh(g.handle, rc.fptr(x), x.shape[1], rc.fptr(t), t.shape[1], n, rc.WEIGHTED, M)
        return
    lib.rnn_bptt_clear_deltas(g.net)
    lib.rnn_amd_set_advance(g.handle)
    if form == "separate":
        lib.rnn_amd_set_opinion(g.handle, rc.fptr(x), x.shape[1], None)
        lib.rnn_amd_set_tanh_error(g.handle, rc.fptr(t), t.shape[1], n)
    else:
        assert form == "opinion_tanh_error"
        lib.rnn_amd_set_opinion_tanh_error(g.handle, rc.fptr(x), x.shape[1], rc.fptr(t), t.shape[1], n)
    lib.rnn_amd_set_calc_deltas(g.handle, 1, None, None)
    lib.rnn_apply_learning(g.net, rc.WEIGHTED, M)


# ------------------------------------------------------------------ 1. the separate kernel --

@pytest.mark.parametrize("hidden,S,n_out,n", [(12, 1, 1, 1), (24, 5, 3, 2), (64, 3, 65, 65), (36, 2, 300, 257)])
def test_separate_kernel_is_the_rule_bit_for_bit(amd, hidden, S, n_out, n):
    lib = amd
    n_in = 7
    g = sc.AmdBatchedSet(lib, input_size=n_in, hidden_size=hidden, output_size=n_out, S=S, D=3, seed=31, learn_rate=1e-3)
    rs = np.random.default_rng([hidden, n_out])
    x = np.ascontiguousarray(rs.uniform(-1, 1, (S, n_in)).astype(F))
    t = np.ascontiguousarray(rs.uniform(-1, 1, (S, n)).astype(F))
    planted = np.zeros((S, g.O), F)
    planted[:, :n_out] = rs.uniform(0.1, 0.3, (S, n_out)).astype(F)
    raw = np.full((S, g.O), np.nan, F)
    g.stats(clear=True)
    lib.rnn_amd_set_advance(g.handle)
    lib.rnn_amd_set_put_o_error(g.handle, rc.fptr(planted), g.O)
    lib.rnn_amd_set_opinion(g.handle, rc.fptr(x), n_in, rc.fptr(raw))
    assert np.isfinite(raw).all() and np.abs(raw[:, :n_out]).max() > 0
    lib.rnn_amd_set_tanh_error(g.handle, rc.fptr(t), n, n)
    snap, st = g.snapshot(), g.stats()
    g.close()
    ans, err, loss = pc.np_rule(raw[:, :n], t)
    assert same(snap["output"][:, :n], ans), "the answers are not dream_tanh of the fetched outputs"
    assert same(snap["o_error"][:, :n], err), "the error is not parrot_error of the answers"
    assert same(snap["output"][:, n:], raw[:, n:]), "outputs from column n on were touched"
    assert same(snap["o_error"][:, n:], planted[:, n:]), "error from column n on was touched"
    want = float(loss.astype(np.float64).sum())
    assert st.count == S and abs(st.error - want) <= RTOL * want, (st.count, st.error, want)


EDGE_N, EDGE_WIDTH = 10, 12


def edge_rows():
    """-> (rows, control rows): symbol rows of EDGE_WIDTH outputs, the first EDGE_N of which take the loss.  Rows 0 and 1
    are clean and hold 0, +-4.97 and its neighbours; rows 2 .. 4 are row 0 with infinities and a NaN among the scored
    outputs and behind them; the control's rows have 0.25 where those are not finite"""
    x = F(4.97)
    base = np.array([0.0, x, np.nextafter(x, F(0)), np.nextafter(x, F(9)), -x, np.nextafter(-x, F(0)), np.nextafter(-x, F(-9)),
                     0.5, -1.5, 3.0, 0.75, -0.125], F)
    other = np.array([0.125, 1.0, -2.0, 4.0, -4.5, 0.25, 1e-3, -1e-3, 2.5, -3.5, 6.0, -7.0], F)
    rows_ = [base, other]
    for entries in (((7, np.inf), (9, -np.inf)), ((8, np.nan),), ((0, -np.inf), (8, np.inf), (11, np.inf))):
        r = base.copy()
        for pos, val in entries:
            r[pos] = val
        rows_.append(r)
    control = [np.where(np.isfinite(r), r, F(0.25)).astype(F) for r in rows_]
    return rows_, control


def edge_step(lib, form, rows_, sym, t):
    S, nsym, hidden = len(sym), len(rows_), 16
    g = sc.AmdBatchedSet(lib, input_size=nsym, hidden_size=hidden, output_size=EDGE_WIDTH, S=S, D=3, seed=3, learn_rate=0.0)
    ih, ho = le.designed_nonfinite_weights(g.I, g.H, g.O, hidden, rows_)
    lib.rnn_amd_sync_host(g.net, rc.RNN_AMD_EVERYTHING)
    rc.view(g.net.contents.ih_weights, g.I, g.H)[:] = ih
    rc.view(g.net.contents.ho_weights, g.H, g.O)[:] = ho
    lib.rnn_amd_host_written(g.net, rc.RNN_AMD_WEIGHTS)
    x = np.zeros((S, nsym), F)
    x[np.arange(S), sym] = 1.0
    lib.rnn_bptt_clear_deltas(g.net)
    lib.rnn_amd_set_advance(g.handle)
    if form == "separate":
        lib.rnn_amd_set_opinion(g.handle, rc.fptr(x), nsym, None)
        lib.rnn_amd_set_tanh_error(g.handle, rc.fptr(t), EDGE_N, EDGE_N)
    else:
        lib.rnn_amd_set_opinion_tanh_error(g.handle, rc.fptr(x), nsym, rc.fptr(t), EDGE_N, EDGE_N)
    lib.rnn_amd_set_calc_deltas(g.handle, 1, None, None)   # (every call returns)
    snap = g.snapshot()
    g.close()
    return snap


@pytest.mark.parametrize("form", ["separate", "one launch"])
def test_clamp_neighbours_infinities_and_nan_on_a_written_net(amd, form):
    """loss_edge_cases' written-row net: each stream's output row is a written one.  The NaN column is NaN in answer and
    error, +-inf gives exactly +-1 and error 0, and everything else -- every other column, row and stream, the written
    outputs behind column n, infinities among them -- equals the control's run on clean rows bit for bit"""
    rows_, control = edge_rows()
    sym = np.array([0, 2, 1, 3, 4, 0, 1], np.int32)
    t = np.ascontiguousarray(np.random.default_rng(9).uniform(-1, 1, (len(sym), EDGE_N)).astype(F))
    p = edge_step(amd, form, rows_, sym, t)
    c = edge_step(amd, form, control, sym, t)
    n = EDGE_N
    for j, s in enumerate(sym):
        row = rows_[s]
        ans, err, _ = pc.np_rule(control[s][:n], t[j])
        assert same(c["output"][j, :n], ans) and same(c["o_error"][j, :n], err), j      # the control is the rule
        nan, inf = np.isnan(row[:n]), np.isinf(row[:n])
        fine = ~(nan | inf)
        assert np.isnan(p["output"][j, :n][nan]).all() and np.isnan(p["o_error"][j, :n][nan]).all(), j
        assert same(p["output"][j, :n][inf], np.sign(row[:n][inf])), j
        assert (p["o_error"][j, :n][inf] == 0).all(), j                              # (a zero of either sign: 0 * diff)
        assert same(p["o_error"][j, :n][inf], pc.np_error(np.sign(row[:n][inf]), t[j][inf])), j
        assert same(p["output"][j, :n][fine], c["output"][j, :n][fine]), j
        assert same(p["o_error"][j, :n][fine], c["o_error"][j, :n][fine]), j
        assert same(p["output"][j, n:EDGE_WIDTH], row[n:]) and same(p["o_error"][j, n:], c["o_error"][j, n:]), j
        if np.isfinite(row).all():
            assert same(p["hidden"][j], c["hidden"][j]) and same(p["output"][j], c["output"][j])
    assert same(p["output"][0, :n], pc.np_rule(rows_[0][:n], t[0])[0])
    assert np.array_equal(np.abs(p["output"][0, 1:7]) == 1, np.array([True, False, True, True, False, True]))


# ------------------------------------------------------------------ 2. one generation against the oracle --

@pytest.mark.parametrize("form", pc.FORMS)
@pytest.mark.parametrize("c", pc.GENERATION_CASES, ids=lambda c: c["name"])
def test_one_generation_from_the_devices_state(amd, c, form):
    lib = amd
    kw = pc.case_kw(c)
    g = sc.AmdBatchedSet(lib, **kw)
    n, S = c["n"], c["S"]
    n_warm = c["D"] + 2
    for gen in range(n_warm):
        x, t, planted = pc.case_data(c, gen)
        generation(lib, g, form, x, t, n, planted)
    o = sc.OracleSet(**kw)
    for attempt in range(4):
        # (a hidden pre-activation within rounding of zero may land on either side in another summation order: such a
        # generation is not a parity case -- tests/test_gpu_callers.py, _rnnca_generation)
        _sync_oracle_to(o, g.snapshot())
        x, t, planted = pc.case_data(c, n_warm + attempt)
        g.stats(clear=True)
        generation(lib, g, form, x, t, n, planted)
        raws, losses = pc.oracle_generation(o, x, t, n, planted)
        sg, so, st = g.snapshot(), o.snapshot(), g.stats()
        if np.array_equal(sg["hidden"] != 0, so["hidden"] != 0):
            break
        _same_mask(sg["hidden"], so["hidden"])
    else:
        raise AssertionError("no generation without a rounding-level mask flip in 4 attempts")
    g.close()
    o.close()
    assert np.abs(raws).max() < 4.0
    assert np.abs(so["o_error"][:, :n]).max() > 0 and (np.abs(so["output"][:, :n]) < 1).all()  # the tanh landed in place
    if planted is not None:
        assert same(sg["o_error"][:, n:c["n_out"]], planted[:, n:]) and (sg["o_error"][:, c["n_out"]:] == 0).all()
    replay.check(sg, so, RTOL, keys=["ih_delta", "ho_delta", "ih_w", "ho_w", "ih_m", "ho_m", "hidden", "output",
                                     "hist", "min_error_factor", "ih_scale"],
                 exact=("index", "generation"))
    # (o_error = slope * (target - answer) cancels against the target: held to the norm bars where a row has hundreds of
    # outputs, element by element where it has a few, as _rnnca_generation holds the sigmoid's)
    replay.check(sg, so, RTOL, keys=["o_error"], exact=(), elementwise=c["n_out"] <= 3)
    want = float(losses.astype(np.float64).sum())
    print("%s, %s: error %.9g, the oracle's terms %.9g, count %d" % (c["name"], form, st.error, want, st.count))
    assert st.count == S
    assert abs(st.error - want) <= RTOL * want, (st.error, want)


# ------------------------------------------------------------------ 3. the saturated net --

@pytest.mark.parametrize("form", ["separate", "opinion_tanh_error"])
def test_saturated_net(amd, form):
    lib, c = amd, pc.SATURATED_CASE
    g = sc.AmdBatchedSet(lib, **pc.case_kw(c))
    write_top_layer(lib, g, pc.saturated_ho(g.H, g.O, g.output_size))
    raw = np.full((c["S"], g.O), np.nan, F)
    for gen in range(c["D"] + 1):
        x, t, _ = pc.case_data(c, gen)
        generation(lib, g, form, x, t, c["n"])
        snap = g.snapshot()
        assert same(np.abs(snap["output"][:, :c["n"]]), np.ones((c["S"], c["n"]), F)), gen
        assert same(snap["output"][:, :c["n"]], np.sign(pc.saturated_ho(g.H, g.O, g.output_size)[0, :c["n"]]) * np.ones((c["S"], 1), F))
        for k in ("o_error", "ho_delta", "ih_delta"):
            assert (snap[k] == 0).all(), (k, gen)          # (zeros of either sign: the slope 0 times a difference)
    lib.rnn_amd_set_opinion(g.handle, rc.fptr(x), x.shape[1], rc.fptr(raw))
    g.close()
    assert np.all(np.abs(raw[:, :c["n"]]) > 4.97 * (1 + 1e-3))


# ------------------------------------------------------------------ 4. one launch against the separate calls --

@pytest.mark.parametrize("between", ["nothing", "put_o_error"])
def test_one_launch_against_separate_calls(amd, between):
    """two sets with the same seed, six generations: rnn_amd_set_opinion_tanh_error on one, rnn_amd_set_opinion +
    rnn_amd_set_tanh_error on the other, at the 2e-5 of test_what_happens_between_the_one_call_loss_and_the_delta_call
    (the one-launch form sums the output layer in another order).  With another output error put between loss and delta
    call on both, a top backprop that wrongly survived would show in the deltas at once."""
    lib = amd
    S, D, NIN, NOUT = 16, 4, 12, 7
    kw = dict(input_size=NIN, hidden_size=64, output_size=NOUT, S=S, D=D, learn_rate=3e-3, seed=52)
    ga, gb = sc.AmdBatchedSet(lib, **kw), sc.AmdBatchedSet(lib, **kw)
    rs = np.random.default_rng(29)
    for step in range(6):
        x = np.ascontiguousarray(rs.uniform(-1, 1, (S, NIN)).astype(F))
        t = np.ascontiguousarray(rs.uniform(-1, 1, (S, NOUT)).astype(F))
        err = (rs.standard_normal((S, ga.O)) * 0.1).astype(F)
        err[:, NOUT:] = 0
        for g, one_call in ((ga, True), (gb, False)):
            lib.rnn_bptt_clear_deltas(g.net)
            lib.rnn_amd_set_advance(g.handle)
            if one_call:
                lib.rnn_amd_set_opinion_tanh_error(g.handle, rc.fptr(x), NIN, rc.fptr(t), NOUT, NOUT)
                assert lib.rnn_amd_set_deferred(g.handle) & TOP_DONE, "the one-launch form did not leave the top backprop done"
            else:
                lib.rnn_amd_set_opinion(g.handle, rc.fptr(x), NIN, None)
                lib.rnn_amd_set_tanh_error(g.handle, rc.fptr(t), NOUT, NOUT)
                assert not lib.rnn_amd_set_deferred(g.handle) & TOP_DONE
            if between == "put_o_error":
                lib.rnn_amd_set_put_o_error(g.handle, rc.fptr(err), g.O)
                assert not lib.rnn_amd_set_deferred(g.handle) & TOP_DONE, "a top backprop survived another output error"
            lib.rnn_amd_set_calc_deltas(g.handle, 1, None, None)
            lib.rnn_apply_learning(g.net, rc.NESTEROV, 0.9)
        sa, sb = ga.snapshot(), gb.snapshot()
        replay.check(sa, sb, 2e-5, keys=["ih_w", "ho_w", "ih_m", "ho_m", "ih_delta", "ho_delta", "hidden", "output", "hist",
                                         "o_error"], exact=("index", "generation"), elementwise=False)
        if between == "put_o_error":
            assert same(sa["o_error"], err) and same(sb["o_error"], err)
    ga.close()
    gb.close()


# ------------------------------------------------------------------ 5. many steps --

def block_frames(T, S, ld, seed):
    return np.ascontiguousarray(np.random.default_rng(seed).uniform(-1, 1, (T + 1, S, ld)).astype(F))


def run_loop(lib, g, frames, n, condition):
    for t in range(len(frames) - 1):
        a, b = np.ascontiguousarray(frames[t]), np.ascontiguousarray(frames[t + 1])
        lib.rnn_amd_set_dense_step_tanh(g.handle, rc.fptr(a), a.shape[1], rc.fptr(b), b.shape[1], n, rc.WEIGHTED, M)
        if condition:
            lib.rnn_condition_net(g.net)


def hold_twins(ga, gb, what):
    sa, sb = ga.snapshot(), gb.snapshot()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]) if sa[k].dtype.kind != "f" else same(sa[k], sb[k]), "%s: %s differs" % (what, k)
    ta, tb = ga.stats(), gb.stats()
    assert (ta.count, ta.error) == (tb.count, tb.error) and ta.count > 0, (what, ta.count, ta.error, tb.count, tb.error)


# hidden, streams, inputs = outputs, ld, depth.  260 outputs are past the top launch: there the many-step call takes its
# other route, the whole forward pass and the separate loss kernel on the block's device rows, ld floats apart
MANY = [(64, 5, 8, 11, 3), (199, 9, 256, 256, 4), (64, 5, 260, 263, 3)]


@pytest.mark.parametrize("hidden,S,width,ld,D", MANY)
def test_many_steps_are_the_loop_of_single_steps(amd, hidden, S, width, ld, D):
    lib = amd
    kw = dict(input_size=width, hidden_size=hidden, output_size=width, S=S, D=D, learn_rate=1e-3, seed=61,
              variance=0.005 if width > 64 else None)
    for T in (1, 3, D + 2):
        ga, gb = sc.AmdBatchedSet(lib, **kw), sc.AmdBatchedSet(lib, **kw)
        frames = block_frames(T, S, ld, [hidden, T])
        ga.stats(clear=True), gb.stats(clear=True)
        assert train_frames(lib, ga, frames, width) == T
        run_loop(lib, gb, frames, width, False)
        hold_twins(ga, gb, "T = %d" % T)
        ga.close()
        gb.close()


def test_blocks_chain_on_their_shared_frame(amd):
    lib = amd
    hidden, S, width, ld, D = MANY[0]
    kw = dict(input_size=width, hidden_size=hidden, output_size=width, S=S, D=D, learn_rate=1e-3, seed=61)
    ga, gb = sc.AmdBatchedSet(lib, **kw), sc.AmdBatchedSet(lib, **kw)
    frames = block_frames(5, S, ld, 77)
    ga.stats(clear=True), gb.stats(clear=True)
    train_frames(lib, ga, frames, width)
    train_frames(lib, gb, frames[:3], width)
    train_frames(lib, gb, frames[2:], width)
    hold_twins(ga, gb, "2 + 3")
    ga.close()
    gb.close()


def test_many_steps_with_conditioning(amd):
    """the net's conditioning flags on (scale and zero), nine generations from generation 0: the scale interval
    (generation % 8 == 0) and the zero interval (== 2) are both crossed"""
    lib = amd
    hidden, S, width, ld, D = MANY[0]
    flags = rc.FLAG_STANDARD | rc.FLAG_ADAPTIVE_MIN_ERROR | rc.COND_USE_SCALE | rc.COND_USE_ZERO
    kw = dict(input_size=width, hidden_size=hidden, output_size=width, S=S, D=D, learn_rate=1e-3, seed=61, flags=flags)
    ga, gb, gc = (sc.AmdBatchedSet(lib, **kw) for _ in range(3))
    frames = block_frames(9, S, ld, 78)
    for g in (ga, gb, gc):
        g.stats(clear=True)
    train_frames(lib, ga, frames, width, condition=True)
    run_loop(lib, gb, frames, width, True)
    run_loop(lib, gc, frames, width, False)
    hold_twins(ga, gb, "conditioned")
    assert int(ga.snapshot()["generation"][0]) == 9
    assert not same(ga.snapshot()["ih_w"], gc.snapshot()["ih_w"]), "the conditioning left no trace: the case shows nothing"
    for g in (ga, gb, gc):
        g.close()


# ------------------------------------------------------------------ 6. the zero-answer net --

def dyadic_targets(c, gen):
    rs = np.random.default_rng([c["seed"], 5000 + gen])
    return rs.choice(np.array([0.0, 0.25, -0.25, 0.5, -0.5, 1.0], F), (c["S"], c["output_size"])).astype(F)


ZERO_KEYS = ["ih_w", "ho_w", "ih_m", "ho_m", "ih_delta", "ho_delta", "hist", "hidden", "output", "o_error", "min_error_factor",
             "ih_scale", "index", "generation"]


def zero_answer_rows(c):
    """-> (the D forward passes' inputs, the training generation's inputs, its dyadic targets)"""
    fill = [np.ascontiguousarray(ec.inputs_of(c, gen), F) for gen in range(c["D"])]
    return fill, np.ascontiguousarray(ec.inputs_of(c, c["D"]), F), np.ascontiguousarray(dyadic_targets(c, c["D"]))


def zero_answer_device_step(lib):
    """exact_cases' zero-answer net of the "sigmoid" case, imported unchanged, on the device: D forward passes that fill the
    ring, then ONE rnn_amd_set_dense_step_tanh (the net is exact for one training generation: its twins diverge at the
    first update).  Every answer is exactly 0, dream_tanh(0) is 0 and the error is exactly the target.  -> the snapshot"""
    from test_gpu_exact_generations import set_kw, write_net
    c = ec.CASES["sigmoid"]
    g = sc.AmdBatchedSet(lib, **set_kw(c))
    write_net(lib, g, c, ec.net_of(c))
    fill, x, t = zero_answer_rows(c)
    for xf in fill:
        lib.rnn_amd_set_advance(g.handle)
        lib.rnn_amd_set_opinion(g.handle, rc.fptr(xf), xf.shape[1], None)
    lib.rnn_amd_set_dense_step_tanh(g.handle, rc.fptr(x), x.shape[1], rc.fptr(t), t.shape[1], t.shape[1], c["method"], ec.MOMENTUM)
    sg = g.snapshot()
    g.close()
    n = c["output_size"]
    assert same(sg["output"][:, :n], np.zeros((c["S"], n), F)) and same(sg["o_error"][:, :n], t)
    return sg


def test_zero_answer_net_equals_the_oracle(amd):
    """one rnn_amd_set_dense_step_tanh with dyadic targets EQUALS the oracle's generation with that o_error written, in every
    element of every array"""
    from test_gpu_exact_generations import set_kw
    c = ec.CASES["sigmoid"]
    sg = zero_answer_device_step(amd)
    net = ec.net_of(c)
    o = sc.OracleSet(**set_kw(c))
    a = o.arrays()
    for k in ("ih_w", "ho_w", "ih_m", "ho_m"):
        a[k][:] = net[k]
    o.z.contents.ho_scale = c["ho_scale"]
    o.z.contents.momentum_weight = ec.MOMENTUM_WEIGHT
    fill, x, t = zero_answer_rows(c)
    for xf in fill:
        for j in range(c["S"]):
            o.orc.orc_advance(o.z, j)
            o.orc.orc_opinion(o.z, j, rc.fptr(np.ascontiguousarray(xf[j])), 0.0)
    raws, _ = pc.oracle_generation(o, x, t, c["output_size"], momentum=ec.MOMENTUM)
    so = o.snapshot()
    o.close()
    assert not raws.any()
    for k in ZERO_KEYS:
        assert np.array_equal(sg[k], so[k]), "%s is not the oracle's" % k


@pytest.mark.skipif(not rc.have_ref(), reason="needs the compiled reference (oracle/_ref, built where the reference's sources are)")
def test_zero_answer_net_equals_the_compiled_reference(amd):
    """the same step EQUALS the compiled reference's generation -- rnn_bptt_advance, rnn_opinion, that o_error written,
    rnn_bptt_calc_deltas per stream, rnn_apply_learning -- in every element of every array"""
    from test_gpu_exact_generations import set_kw
    c = ec.CASES["sigmoid"]
    sg = zero_answer_device_step(amd)
    net = ec.net_of(c)
    ref = sc.ApiSet(rc.load_ref(), **set_kw(c))
    rl = ref.lib
    n0, b0 = ref.net.contents, ref.net.contents.bptt.contents
    for ptr, k, shape in ((n0.ih_weights, "ih_w", (ref.I, ref.H)), (n0.ho_weights, "ho_w", (ref.H, ref.O)),
                          (b0.ih_momentum, "ih_m", (ref.I, ref.H)), (b0.ho_momentum, "ho_m", (ref.H, ref.O))):
        rc.view(ptr, *shape)[:] = net[k]
    b0.ho_scale = c["ho_scale"]
    b0.momentum_weight = ec.MOMENTUM_WEIGHT
    fill, x, t = zero_answer_rows(c)
    for xf in fill:
        for j in range(ref.S):
            rl.rnn_bptt_advance(ref.nets[j])
            rl.rnn_opinion(ref.nets[j], rc.fptr(np.ascontiguousarray(xf[j])), 0.0)
    n = c["output_size"]
    rl.rnn_bptt_clear_deltas(ref.net)
    for j in range(ref.S):
        rl.rnn_bptt_advance(ref.nets[j])
        rl.rnn_opinion(ref.nets[j], rc.fptr(np.ascontiguousarray(x[j])), 0.0)
        e = rc.view(ref.nets[j].contents.bptt.contents.o_error, ref.O)
        e[:] = 0
        e[:n] = t[j]
        rl.rnn_bptt_calc_deltas(ref.nets[j], 1, None)
    rl.rnn_apply_learning(ref.net, c["method"], ec.MOMENTUM)
    sr = ref.snapshot()
    ref.close()
    for k in ZERO_KEYS:
        assert np.array_equal(sg[k], sr[k]), "%s is not the compiled reference's" % k


# ------------------------------------------------------------------ 7. learning, through the tool --

def test_the_tool_learns_and_the_player_plays_its_net(amd, tmp_path):
    L = pc.LEARN
    build = os.path.join(rc.ROOT, "build")
    features, netfile, dream = str(tmp_path / "features.f32"), str(tmp_path / "parrot.net"), str(tmp_path / "dream.f32")
    pc.learning_frames().tofile(features)
    r = subprocess.run([os.path.join(build, "parrot_train_amd"), "-c", str(L["channels"]), "-H", str(L["hidden"]), "-d",
                        str(L["depth"]), "-r", str(L["rate"]), "-b", str(L["block"]), "-s", str(L["seed"]), features, netfile],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln.split() for ln in r.stdout.strip().splitlines()]
    print(r.stdout)
    assert len(lines) == L["generations"] // L["block"] and int(lines[-1][0]) == L["generations"]
    first, last = float(lines[0][1]), float(lines[-1][1])
    assert np.isfinite(first) and np.isfinite(last) and last < 0.5 * first, (first, last)
    frames = 6
    r = subprocess.run([os.path.join(build, "parrot_dream_amd"), "-c", str(L["channels"]), "-n", str(frames), "-z", "0",
                        netfile, dream], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.fromfile(dream, F)
    assert got.size == frames * L["channels"] * 256 and np.isfinite(got).all() and np.abs(got).max() <= 1
