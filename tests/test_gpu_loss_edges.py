"""Every training loss of the device against the oracle OUTSIDE the softmax's window: output rows with a non-zero shift
(all three branches), fast_expf loops of 0 to 6 rounds, denormal and zero likelihoods, the -100 cap, ties for the best
guess across lanes and waves, and fast_sigmoid from -1e4 to 1e4 -- on a net whose output rows are written, not learned
(tests/loss_edge_cases.py; the CPU half, tests/test_loss_edge_rows.py, shows that the oracle is sound there, what each case
below reaches, and that the rows would notice a slip in any one rule).

Eleven kernels or instances: k_text_top2, k_text_top<0> (the text step, narrow and wide), k_softmax_error (stand-alone),
k_multi_softmax_error (heads), k_grouped_softmax_error and k_text_top<2> (class groups), k_sigmoid_mse_error, k_text_top<1>
and k_sigmoid_outputs (sigmoid), k_xent_accumulate and k_multi_xent_accumulate (cross entropy).

What is held: the device's output row equals the written row bit for bit; o_error within 1e-4 of the oracle's on EVERY
element, no magnitude floor (the inputs are exact), and denormal or zero where the oracle's is; count / correct / trained /
wins / generator states exact; error and entropy sums to 1e-4; the deltas, ih_scale, min_error_factor, the history and the
hidden rows through replay.check at 1e-4.

MEASURED on the MI355X, the largest distance of o_error (for the sigmoid cases also of the answers in place) from the
oracle's in units in the last place, per case: 0 everywhere -- k_text_top<0> at 65, 130 and 256 outputs, k_softmax_error at
42, 65, 130 and 300, k_multi_softmax_error at 5 x 3, 24 x 4, 73 x 3 and 128 x 2 with leakage 0 and 0.35, both class-group
forms with and without weights, the three sigmoid forms at n = 3 and 16 -- except k_text_top2: 4 ulps at 42 outputs, 7 ulps
at 64.  That kernel adds the exponentials as a tree over the lanes where the reference adds in index order
(text_softmax_regs, kernels_loss.hip, which says so): 7 ulps are 8e-7 of the value, a hundredth of the bar.  The cases
that measured 0 assert bit equality; the two k_text_top2 cases assert the bar.  The cross-entropy sums agree to 5e-8.

One thing the construction does not make exact: the HIDDEN error of a row whose logits are all equal (`all_m1000`) is
-1000 sum(e), and sum(e) is zero but for rounding.  Whether that is 0 or 6e-5 is the summation order's to decide, and the
BPTT loop's exit asks exactly that (cancelled_streams below).  At 64 outputs the device's sum is 0 and the oracle's is not,
so that stream runs one level less deep and its min_error_factor takes another step: min_error_factor is held on every
stream whose hidden error did not cancel, everything else on all of them.
"""
import ctypes as C

import numpy as np
import pytest

import loss_edge_cases as le
import recur_ctypes as rc
import replay
import scenarios as sc

pytestmark = pytest.mark.gpu
RTOL = 1e-4
F = np.float32
HIDDEN = 64

# The largest o_error difference in ulps measured per case on the MI355X.  Every case that is not listed measured 0 and
# asserts bit equality.  k_text_top2 adds the exponentials as a tree over the lanes, not in the reference's index order
# (text_softmax_regs, kernels_loss.hip: by design, and said there), so its likelihoods are a few ulps off: the bar holds them.
ULPS = {"text step 42": 4, "text step 64": 7, "text step 42, weights": 4}


@pytest.fixture(scope="module")
def amd():
    lib = rc.load_amd()
    assert lib.rnn_amd_device_count() >= 1, "no HIP device: the product has no CPU fallback"
    rc.bind_char(lib)
    return lib


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def designed(lib, symbol_rows, input_size, output_size, S, D=4, hidden_size=HIDDEN, learn_rate=0.0, batched=True):
    """the designed net on the device and on the oracle: the same written weights, zero momentum, the same generators"""
    kw = dict(input_size=input_size, hidden_size=hidden_size, output_size=output_size, S=S, D=D, learn_rate=learn_rate,
              seed=3)
    g = (sc.AmdBatchedSet if batched else sc.ApiSet)(lib, **kw)
    o = sc.OracleSet(**kw)
    ih, ho = le.designed_weights(g.I, g.H, g.O, hidden_size, symbol_rows)
    assert (g.I, g.H, g.O) == (o.I, o.H, o.O)
    n0, b0 = g.net.contents, g.net.contents.bptt.contents
    lib.rnn_amd_sync_host(g.net, rc.RNN_AMD_EVERYTHING)
    rc.view(n0.ih_weights, g.I, g.H)[:] = ih
    rc.view(n0.ho_weights, g.H, g.O)[:] = ho
    rc.view(b0.ih_momentum, g.I, g.H)[:] = 0
    rc.view(b0.ho_momentum, g.H, g.O)[:] = 0
    lib.rnn_amd_host_written(g.net, rc.RNN_AMD_WEIGHTS | rc.RNN_AMD_MOMENTUMS)
    a = o.arrays()
    a["ih_w"][:] = ih
    a["ho_w"][:] = ho
    for k in ("ih_m", "ho_m", "ih_aux", "ho_aux"):
        a[k][:] = 0
    snap = g.snapshot()
    assert np.array_equal(snap["ih_w"], ih) and np.array_equal(snap["ho_w"], ho)
    for j in range(S):
        r = o.z.contents.rng[j]
        r.a, r.b, r.c, r.d = (int(x) for x in snap["rng"][j])
    return g, o


class Worst:
    """the largest o_error distance of a case in ulps: printed, and held to what was measured"""

    def __init__(self, case):
        self.case, self.ulps = case, 0

    def hold(self, dev, orc, what="o_error"):
        dev, orc = np.ascontiguousarray(dev, np.float32), np.ascontiguousarray(orc, np.float32)
        assert dev.shape == orc.shape and np.isfinite(orc).all()
        assert np.isfinite(dev).all(), "%s: %s is not finite on the device" % (self.case, what)
        u = le.ulps(dev, orc)
        self.ulps = max(self.ulps, int(u.max()))
        if ULPS.get(self.case, 0) == 0:
            assert np.array_equal(dev, orc) and int(u.max()) == 0, "%s: %s differs by %d ulps" % (self.case, what, u.max())
            return
        tiny = np.abs(orc) < le.TINY  # the oracle's value denormal or zero: so is the device's
        assert (np.abs(dev[tiny]) < le.TINY).all(), "%s: %s not denormal or zero where the oracle's is" % (self.case, what)
        d, bound = np.abs(dev.astype(np.float64) - orc)[~tiny], RTOL * np.abs(orc.astype(np.float64))[~tiny]
        worst = (d / np.abs(orc.astype(np.float64))[~tiny]).max() if d.size else 0.0
        assert (d <= bound).all(), "%s: %s off by %.3g of itself (%d ulps)" % (self.case, what, worst, u.max())

    def report(self):
        print("%s: largest o_error difference %d ulps" % (self.case, self.ulps))


DELTA_KEYS = ["ih_delta", "ho_delta", "ih_scale", "min_error_factor", "hist", "hidden"]


def cancelled_streams(so):
    """Streams whose hidden error is what rounding leaves of a sum that cancels: an active unit's |sum of w e| below 1e-4
    of its sum of |w e| (float64, from the oracle's own arrays).  A row of equal logits c has the hidden error c sum(e),
    and sum(e) is 0 but for the softmax's rounding: 6e-8 x 1000 on `all_m1000`, exactly 0 or not by the order of the sum.
    The BPTT loop's exit `error_sum <= 1e-8 top_error_sum` (recur-nn.c:387) asks whether that is above 1e-8: the executed
    depth, and with it the adaptive min_error_factor's step of 1e-3 per level, is then the summation order's to decide."""
    ho, hid, err = so["ho_w"].astype(np.float64), so["hidden"], so["o_error"].astype(np.float64)
    out = np.zeros(len(hid), bool)
    for j in range(len(hid)):
        for y in np.nonzero(hid[j, 1:])[0] + 1:
            terms = ho[y] * err[j]
            out[j] |= bool(abs(terms.sum()) < RTOL * np.abs(terms).sum())
    return out


def hold_deltas(o, sg, so, exact=("index", "generation"), keys=None):
    """replay.check at the parity bar, as the neighbouring tests do.  min_error_factor of a stream whose hidden error
    cancelled (see above) is not held, on that stream only: the oracle then goes on from the device's value."""
    lost = cancelled_streams(so)
    if lost.any():
        print("hidden error cancelled on streams %s: min_error_factor %s on the device, %s on the oracle"
              % (np.nonzero(lost)[0], sg["min_error_factor"][lost], so["min_error_factor"][lost]))
    assert lost.sum() <= len(lost) // 3, "too many streams' hidden errors cancel: %s" % np.nonzero(lost)[0]
    if lost.any():
        assert np.all(np.abs(sg["min_error_factor"][lost] / so["min_error_factor"][lost] - 1) < 4e-3 * o.D)
        so = dict(so)
        so["min_error_factor"] = np.where(lost, sg["min_error_factor"], so["min_error_factor"])
        o.arrays()["min_error_factor"][:] = so["min_error_factor"]
    replay.check(sg, so, RTOL, keys=keys or DELTA_KEYS, exact=exact)


def hold_outputs(sg, plan_rows):
    for j, row in enumerate(plan_rows):
        assert np.array_equal(_bits(sg["output"][j, :len(row)]), _bits(row)), "stream %d: the output row is not the written one" % j


def close_stats(got, want):
    assert abs(got - want) <= RTOL * abs(want), (got, want)


# ------------------------------------------------------------------ the text step --

@pytest.mark.parametrize("n", le.TEXT_NARROW + le.TEXT_WIDE)
def test_text_step(amd, n):
    """rnn_amd_set_char_step: k_text_top2 (o_size up to 64), k_text_top<0> (up to 256); every (row, target) on some stream"""
    named = le.symbol_rows(n)
    pairs, _ = le.pairs_of(named)
    S = 12
    g, o = designed(amd, [r for _, r in named], n, n, S)
    text, positions, plan = le.stream_text(pairs, S)
    w = Worst("text step %d" % n)
    g.stats(clear=True)
    for k, i in enumerate(positions):
        g.char_step(text, i, rc.WEIGHTED, 0.9)
        o.char_step(text, i, rc.WEIGHTED, 0.9)
        sg, so = g.snapshot(), o.snapshot()
        hold_outputs(sg, [named[c][1] for c, _ in plan[k]])
        assert np.array_equal(_bits(so["output"]), _bits(sg["output"]))
        w.hold(sg["o_error"], so["o_error"])
        hold_deltas(o, sg, so)
        assert np.array_equal(sg["ih_w"], so["ih_w"]) and np.array_equal(sg["ho_w"], so["ho_w"])  # learn rate 0: as written
    st, z = g.stats(), o.z.contents
    assert st.count == z.stat_count == S * len(positions) and st.correct == z.stat_correct  # (ties: the lowest index)
    assert 0 < st.correct < st.count
    close_stats(st.error, z.stat_error)
    close_stats(st.entropy, z.stat_entropy)
    w.report()
    g.close()
    o.close()


@pytest.mark.parametrize("n", [42, 130])
def test_text_step_moves_the_weights_as_the_oracle_does(amd, n):
    """ONE step with learn rate 1e-5: the update that the edge rows' error leads to, weights and momentum"""
    named = le.symbol_rows(n)
    pairs, _ = le.pairs_of(named)
    S = 12
    g, o = designed(amd, [r for _, r in named], n, n, S, learn_rate=1e-5)
    # the rows that leave the window, each against its least likely symbol
    picked = [(c, int(np.argmin(row))) for c, (_, row) in enumerate(named)][1:S + 1]
    picked = [p if p in pairs else (p[0], int(np.argmax(named[p[0]][1]))) for p in picked]
    text, positions, plan = le.stream_text(picked, S)
    g.char_step(text, 0, rc.WEIGHTED, 0.9)
    o.char_step(text, 0, rc.WEIGHTED, 0.9)
    sg, so = g.snapshot(), o.snapshot()
    w = Worst("text step %d, weights" % n)
    w.hold(sg["o_error"], so["o_error"])
    w.report()
    assert not np.array_equal(so["ho_w"], le.designed_weights(o.I, o.H, o.O, HIDDEN, [r for _, r in named])[1])
    hold_deltas(o, sg, so, keys=["ih_w", "ho_w", "ih_m", "ho_m"] + DELTA_KEYS)
    g.close()
    o.close()


# ------------------------------------------------------------------ the stand-alone loss --

@pytest.mark.parametrize("n", le.ALONE)
def test_stand_alone_loss(amd, n):
    """rnn_amd_set_one_hot_opinion + rnn_amd_set_softmax_error + rnn_amd_set_calc_deltas: k_softmax_error"""
    named = le.symbol_rows(n)
    pairs, _ = le.pairs_of(named)
    S = 12
    g, o = designed(amd, [r for _, r in named], 24, n, S)
    w = Worst("stand-alone %d" % n)
    g.stats(clear=True)
    err_sum, ent_sum, correct = 0.0, 0.0, 0
    plan = le.share_out(pairs, S)
    for step in plan:
        hot = np.array([c for c, _ in step], np.int32)
        tgt = np.array([t for _, t in step], np.int32)
        amd.rnn_amd_set_advance(g.handle)
        amd.rnn_amd_set_one_hot_opinion(g.handle, rc.iptr(hot), None)
        amd.rnn_amd_set_softmax_error(g.handle, rc.iptr(tgt))
        amd.rnn_amd_set_calc_deltas(g.handle, 0, None, None)
        for j in range(S):
            hit = C.c_int(0)
            o.orc.orc_advance(o.z, j)
            e = o.orc.orc_net_error_bptt(o.z, j, int(hot[j]), int(tgt[j]), C.byref(hit))
            err_sum += e
            ent_sum += o.orc.orc_capped_log2f(F(1) - F(e))
            correct += hit.value
            o.orc.orc_calc_deltas(o.z, j, 1 if j else 0, None)
        sg, so = g.snapshot(), o.snapshot()
        hold_outputs(sg, [named[c][1] for c, _ in step])
        w.hold(sg["o_error"], so["o_error"])
        hold_deltas(o, sg, so)
    st = g.stats()
    assert st.count == S * len(plan) and st.correct == correct and 0 < correct < st.count
    close_stats(st.error, err_sum)
    close_stats(st.entropy, ent_sum)
    w.report()
    g.close()
    o.close()


# ------------------------------------------------------------------ heads --

@pytest.mark.parametrize("leakage", [0.0, 0.35])
@pytest.mark.parametrize("alen,heads", le.HEADS)
def test_heads(amd, alen, heads, leakage):
    """rnn_amd_set_multi_step: k_multi_softmax_error, a head's outputs in registers (up to 128) -- every catalogue row as
    the stream's own head against each of its targets, and (leakage 0.35) as a leaked head too"""
    full, triples, slots = le.head_case(alen, heads)
    S = 12
    g, o = designed(amd, full, alen, alen * heads, S)
    w = Worst("heads %d x %d, leakage %g" % (alen, heads, leakage))
    g.stats(clear=True)
    err_sum, ent_sum, leaked = 0.0, 0.0, 0
    plan = le.share_out(triples, S)
    ranges = (C.c_int * (2 * (heads + 1)))()
    for step in plan:
        hot = np.array([c for c, _, _ in step], np.int32)
        cls = np.array([h for _, h, _ in step], np.int32)
        nxt = np.array([t for _, _, t in step], np.int32)
        amd.rnn_amd_set_multi_step(g.handle, rc.iptr(hot), rc.iptr(nxt), rc.iptr(cls), alen, leakage, rc.WEIGHTED, 0.9)
        for j in range(S):
            o.orc.orc_advance(o.z, j)
            e = o.orc.orc_multi_softmax_error(o.z, j, int(hot[j]), int(nxt[j]), int(cls[j]), alen, leakage, ranges)
            err_sum += e
            ent_sum += o.orc.orc_capped_log2f(F(1) - F(e))
            o.orc.orc_calc_deltas(o.z, j, 1 if j else 0, ranges)
        o.orc.orc_apply_learning(o.z, rc.WEIGHTED, 0.9)
        sg, so = g.snapshot(), o.snapshot()
        hold_outputs(sg, [full[c] for c in hot])
        w.hold(sg["o_error"], so["o_error"])
        trained = np.abs(so["o_error"][:, :alen * heads]).reshape(S, heads, alen).sum(axis=2) > 0
        leaked += int(trained.sum()) - int(trained[np.arange(S), cls].sum())
        hold_deltas(o, sg, so, exact=("index", "generation", "rng"))
    assert (leaked > 0) == (leakage > 0)
    st = g.stats()
    assert st.count == S * len(plan)
    close_stats(st.error, err_sum)
    close_stats(st.entropy, ent_sum)
    w.report()
    g.close()
    o.close()


# ------------------------------------------------------------------ class groups --

@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("one_call", [False, True])
def test_class_groups(amd, one_call, weighted):
    """rnn_amd_set_opinion + rnn_amd_set_grouped_softmax_error (k_grouped_softmax_error) and
    rnn_amd_set_opinion_grouped_softmax (k_text_top<2>): groups of 1, 2, 3, 7 and 30 outputs, the one-hot fed as floats"""
    full, goff, gsize, slots = le.group_case()
    S = nsym = len(full)
    n_out = int(gsize.sum())
    ng = len(gsize)
    assert S % 4 == 0
    g, o = designed(amd, full, nsym, n_out, S)
    weight = np.ascontiguousarray(np.linspace(0.25, 2.0, g.O, dtype=np.float32)) if weighted else None
    wp = rc.fptr(weight) if weighted else None
    w = Worst("class groups, %s, %s" % ("one call" if one_call else "two calls", "weighted" if weighted else "plain"))
    g.stats(clear=True)
    wins, wrong, groups = C.c_int(0), C.c_float(0), 0
    wrong_sum = 0.0
    for step in range(5):
        sym = (np.arange(S) + step) % nsym
        x = np.zeros((S, nsym), np.float32)
        x[np.arange(S), sym] = 1.0
        tg = np.ascontiguousarray(le.group_targets(slots, step)[sym])
        if step == 3:
            tg[2, :] = -1  # a stream with nothing to train
        trained = np.zeros(S, np.uint8)
        amd.rnn_bptt_clear_deltas(g.net)
        amd.rnn_amd_set_advance(g.handle)
        if one_call:
            amd.rnn_amd_set_opinion_grouped_softmax(g.handle, rc.fptr(x), nsym, ng, rc.iptr(goff), rc.iptr(gsize), rc.iptr(tg),
                                                    wp, rc.u8ptr(trained))
        else:
            amd.rnn_amd_set_opinion(g.handle, rc.fptr(x), nsym, None)
            amd.rnn_amd_set_grouped_softmax_error(g.handle, ng, rc.iptr(goff), rc.iptr(gsize), rc.iptr(tg), wp,
                                                  rc.u8ptr(trained))
        amd.rnn_amd_set_calc_deltas(g.handle, 1, None, rc.u8ptr(trained))
        o.orc.orc_clear_deltas(o.z)
        want_trained = np.zeros(S, np.uint8)
        for j in range(S):
            o.orc.orc_advance(o.z, j)
            o.orc.orc_opinion(o.z, j, rc.fptr(np.ascontiguousarray(x[j])), 0.0)
            wrong.value = 0.0
            k = o.orc.orc_grouped_softmax_error(o.z, j, ng, rc.iptr(goff), rc.iptr(gsize),
                                                rc.iptr(np.ascontiguousarray(tg[j])), wp, C.byref(wins), C.byref(wrong))
            wrong_sum += wrong.value
            groups += k
            want_trained[j] = k > 0
            if k:
                o.orc.orc_calc_deltas(o.z, j, 1, None)
        sg, so = g.snapshot(), o.snapshot()
        hold_outputs(sg, [full[c] for c in sym])
        assert np.array_equal(trained, want_trained)
        w.hold(sg["o_error"], so["o_error"])  # (an untrained group's error is zeros, a stream without any a row of them)
        hold_deltas(o, sg, so)
    st = g.stats()
    assert st.count == groups and st.correct == wins.value and 0 < wins.value < groups
    close_stats(st.error, wrong_sum)
    w.report()
    g.close()
    o.close()


# ------------------------------------------------------------------ sigmoid --

@pytest.mark.parametrize("n", [3, le.SIGMOID_WIDTH])
@pytest.mark.parametrize("form", ["two calls", "one call", "forward only"])
def test_sigmoid(amd, form, n):
    """rnn_amd_set_sigmoid_mse_error (k_sigmoid_mse_error), rnn_amd_set_opinion_sigmoid_mse (k_text_top<1>),
    rnn_amd_set_sigmoid_outputs (k_sigmoid_outputs): the sigmoid arguments as the designed output rows, -1e4 to 1e4"""
    full = le.sigmoid_case(n)
    S = nsym = len(full)
    width = le.SIGMOID_WIDTH
    g, o = designed(amd, full, nsym, width, S)
    w = Worst("sigmoid %s, n = %d" % (form, n))
    rs = np.random.default_rng(n)
    for step in range(2):
        sym = (np.arange(S) + step) % nsym
        x = np.zeros((S, nsym), np.float32)
        x[np.arange(S), sym] = 1.0
        tgt = np.ascontiguousarray((rs.integers(0, 256, (S, n)) / F(255)).astype(np.float32))
        amd.rnn_bptt_clear_deltas(g.net)
        amd.rnn_amd_set_advance(g.handle)
        if form == "forward only":
            out = np.zeros((S, g.O), np.float32)
            amd.rnn_amd_set_opinion(g.handle, rc.fptr(x), nsym, None)
            amd.rnn_amd_set_sigmoid_outputs(g.handle, n, rc.fptr(out))
        elif form == "one call":
            amd.rnn_amd_set_opinion_sigmoid_mse(g.handle, rc.fptr(x), nsym, rc.fptr(tgt), n, n)
        else:
            amd.rnn_amd_set_opinion(g.handle, rc.fptr(x), nsym, None)
            amd.rnn_amd_set_sigmoid_mse_error(g.handle, rc.fptr(tgt), n, n)
        if form != "forward only":
            amd.rnn_amd_set_calc_deltas(g.handle, 1, None, None)
        o.orc.orc_clear_deltas(o.z)
        for j in range(S):
            o.orc.orc_advance(o.z, j)
            o.orc.orc_opinion(o.z, j, rc.fptr(np.ascontiguousarray(x[j])), 0.0)
            if form == "forward only":
                ans = o.arrays()["output"][j]
                for i in range(n):
                    ans[i] = o.orc.orc_fast_sigmoid(float(ans[i]))
            else:
                o.orc.orc_sigmoid_mse_error(o.z, j, rc.fptr(np.ascontiguousarray(tgt[j])), n)
                o.orc.orc_calc_deltas(o.z, j, 1, None)
        sg, so = g.snapshot(), o.snapshot()
        answers = so["output"][:, :n]
        assert (answers == 0).any() and (answers == 1).any() and ((answers > 0) & (answers < 1)).any()
        w.hold(sg["output"][:, :n], answers, "the sigmoid in place")
        for j, c in enumerate(sym):  # ... and what lies behind the first n outputs is the written row still
            assert np.array_equal(_bits(sg["output"][j, n:width]), _bits(full[c][n:]))
        if form == "forward only":
            w.hold(out[:, :n], answers, "the answers fetched")
            replay.check(sg, so, RTOL, keys=["hidden", "hist"], exact=("index", "generation"))
        else:
            w.hold(sg["o_error"], so["o_error"])
            assert np.abs(so["o_error"]).max() > 0
            hold_deltas(o, sg, so)
    w.report()
    g.close()
    o.close()


# ------------------------------------------------------------------ cross entropy --

def test_cross_entropy_of_a_text_that_walks_every_row(amd):
    """rnn_char_cross_entropy: k_xent_accumulate, the cap on the likelihood itself"""
    alen, heads = le.XENT[0]
    full, text, slots, _ = le.xent_case(alen, heads)
    g, o = designed(amd, full, alen, alen, 1, D=1, batched=False)
    for skip in (0, 5):
        got = amd.rnn_char_cross_entropy(g.net, None, rc.u8ptr(text), len(text), skip, None, 0)
        want = o.orc.orc_cross_entropy(o.z, 0, rc.u8ptr(text), len(text), skip)
        print("cross entropy %d, skip %d: %.9g against %.9g" % (alen, skip, got, want))
        assert 10.0 < want < 100.0  # (capped terms of 100 among ordinary ones)
        assert abs(got - want) <= RTOL * abs(want), (got, want)
    g.close()
    o.close()


def test_cross_entropy_per_head_of_a_text_that_walks_every_row(amd):
    """rnn_char_multi_cross_entropy: k_multi_xent_accumulate, 3 heads of 73"""
    alen, heads = le.XENT[1]
    full, text, slots, _ = le.xent_case(alen, heads)
    g, o = designed(amd, full, alen, alen * heads, 1, D=1, hidden_size=96, batched=False)
    ent_g = (C.c_double * heads)(*([0.0] * heads))
    ent_o = (C.c_double * heads)(*([0.0] * heads))
    amd.rnn_char_multi_cross_entropy(g.net, rc.u8ptr(text), len(text), alen, ent_g, 3)
    o.orc.orc_multi_cross_entropy(o.z, 0, rc.u8ptr(text), len(text), alen, ent_o, 3)
    for h in range(heads):
        print("cross entropy head %d: %.9g against %.9g" % (h, ent_g[h], ent_o[h]))
        assert 10.0 < ent_o[h] < 100.0
        assert abs(ent_g[h] - ent_o[h]) <= RTOL * abs(ent_o[h]), (h, ent_g[h], ent_o[h])
    g.close()
    o.close()
