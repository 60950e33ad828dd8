"""Drivers of tests/test_gpu_scalars.py: the training scalars a caller writes into the public structs BETWEEN calls
(bptt->ho_scale, ->momentum_weight, ->learn_rate, ->momentum, the bottom layer's learn_rate_scale,
net->presynaptic_noise, the momentum argument), moved on the device set and on the oracle alike, and a float64
restatement of the seven update rules for the element-by-element identity.

A *site* names how one generation is driven on both sides (device_step / oracle_step); a *scalar* names what is moved
(moves()).  The same tables drive the device cases and the CPU-only guard that proves from the oracle alone that each
move matters.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

import recur_ctypes as rc
import replay
import scenarios as sc

RTOL = 1e-4
KEYS = ["ih_delta", "ho_delta", "ih_w", "ho_w", "ih_m", "ho_m", "hidden", "output", "o_error", "hist",
        "min_error_factor", "ih_scale"]
BOTTOM_KEYS = ["b_w", "b_m", "b_delta"]
AUX_FLAGS = rc.FLAG_STANDARD | rc.FLAG_ADAPTIVE_MIN_ERROR | rc.FLAG_AUX_ARRAYS
NEEDS_AUX = (rc.ADADELTA, rc.RPROP)
BALLAST = 50.0                       # ADAGRAD from zero accumulators is 0 / sqrt 0 on both sides
AUX_START = 1e-4                     # RPROP's first step sizes (golden case relu_rprop)
MULTI_LEAKAGE = 0.2                  # the multi-head sites: input_size symbols per head, output_size / input_size heads

# comparisons made by one_generation() and how many of them took the next generation because of a rounding-level mask
# flip: the module's last test holds the second to a twentieth of the first
COUNTS = {"comparisons": 0, "retried": 0, "flipped": 0, "values": 0}


# --------------------------------------------------------------------------------------------------- the scalars --

def rule_ignores(scalar, method, site="char_step"):
    """The table of "this scalar cannot matter here", by the rules' definitions (recur-nn.c:601-678): only the weighted
    momentum rule reads momentum_weight (SIMPLIFIED and CLASSICAL compute their own, the others have none), and
    rnn_bptt_calculate's rule is always the weighted one."""
    if scalar == "momentum_weight":
        return site != "calculate" and method != rc.WEIGHTED
    if scalar == "ho_scale":         # apply_sgd_top_layer takes the plain rate (recur-nn.c:927), the recurrent layer's too
        return site == "calculate"
    return False


def moves(scalar, kw):
    """[first move, second move (another value, not the default), the creation value]"""
    lr = np.full(kw["S"], kw.get("learn_rate", 1e-3), np.float32)
    if scalar == "ho_scale":
        return [0.3, 2.5, 1.0]
    if scalar == "momentum_weight":
        return [0.8, 0.1, 0.5]
    if scalar == "momentum":
        return [0.5, 0.8, 0.95]
    if scalar == "learn_rate":       # charmodel-predict.c:107 cuts the prototype's only; the schedule cuts again
        a = lr.copy()
        a[0] *= 0.5
        return [a, a * np.float32(0.5), lr]
    if scalar == "clone_rate":       # the clones' only: stream 0's (the update's rate) stays
        a = lr.copy()
        a[1:] *= 0.25
        b = lr.copy()
        b[1:] *= 4.0
        return [a, b, lr]
    if scalar == "bottom_rate_scale":
        return [0.25, 3.0, kw.get("bottom_rate_scale", 1.0)]
    if scalar == "noise":            # char_epoch.c's adjust_noise halves it
        n = kw["noise"]
        return [n * 0.5, n * 0.25, n]
    raise KeyError(scalar)


def write_scalar(scalar, value, g=None, o=None, state=None):
    """the way a caller does it: fields of the public structs (the prototype's, for what rnn_apply_learning reads)"""
    if scalar == "momentum":
        state["momentum"] = float(value)
        return
    if g is not None:
        b0 = g.nets[0].contents.bptt.contents
        if scalar == "ho_scale":
            b0.ho_scale = value
        elif scalar == "momentum_weight":
            b0.momentum_weight = value
        elif scalar in ("learn_rate", "clone_rate"):
            for j in range(g.S):
                g.nets[j].contents.bptt.contents.learn_rate = float(value[j])
        elif scalar == "bottom_rate_scale":
            g.nets[0].contents.bottom_layer.contents.learn_rate_scale = value
        elif scalar == "noise":
            for j in range(g.S):
                g.nets[j].contents.presynaptic_noise = value
    if o is not None:
        z = o.z.contents
        if scalar == "ho_scale":
            z.ho_scale = value
        elif scalar == "momentum_weight":
            z.momentum_weight = value
        elif scalar in ("learn_rate", "clone_rate"):
            o.arrays()["learn_rate"][:] = value
        elif scalar == "bottom_rate_scale":
            z.b_learn_rate_scale = value
        elif scalar == "noise":
            z.presynaptic_noise = value


# ----------------------------------------------------------------------------------------------------- the sites --

def _text(alphabet=42):
    t = sc.synthetic_text(30000)
    return t if alphabet >= 42 else t % alphabet


def _case_text(site, kw):
    if site == "multi":
        return _text()
    return _text(min(kw.get("bottom_inputs") or kw["input_size"], kw["output_size"]))


def _multi_inputs(i, S, A, NC):
    rs = np.random.default_rng(1000 + i)
    return (rs.integers(0, A, S).astype(np.int32), rs.integers(0, A, S).astype(np.int32),
            rs.integers(0, NC, S).astype(np.int32))


def _taps(text, i, S):
    """the streams' text positions in generation i (charmodel-predict.c:288-300)"""
    L = len(text)
    spacing = (L - 1) // S
    off = (i + np.arange(S) * spacing) % (L - 1)
    return np.ascontiguousarray(text[off].astype(np.int32)), np.ascontiguousarray(text[off + 1].astype(np.int32))


def device_step(site, lib, g, text, i, method, momentum, batch=1):
    if site == "char_step":            # rnn_amd_set_char_step: deltas and update in one call (set_step)
        g.char_step(text, i, method, momentum)
    elif site == "deltas_apply":       # rnn_amd_set_calc_deltas leaves K planes (e->kept); rnn_apply_learning adds them up
        hot, tgt = _taps(text, i, g.S)
        lib.rnn_amd_set_advance(g.handle)
        lib.rnn_amd_set_one_hot_opinion(g.handle, rc.iptr(hot), None)
        lib.rnn_amd_set_softmax_error(g.handle, rc.iptr(tgt))
        lib.rnn_amd_set_calc_deltas(g.handle, 0, None, None)
        lib.rnn_apply_learning(g.net, method, momentum)
    elif site == "pernet":             # the reference's own call sequence, one net at a time
        sc.ApiSet.char_step(g, text, i, method, momentum)
    elif site == "calculate":          # rnn_bptt_calculate: k_fused_updates
        lib.rnn_bptt_advance(g.net)
        g.net_error_bptt(0, int(text[i]), int(text[i + 1]))
        g.net.contents.bptt.contents.momentum = momentum
        lib.rnn_bptt_calculate(g.net, batch)
    elif site == "multi":              # rnn_amd_set_multi_step: set_step through its own StepSpec
        A = g.input_size
        hot, nxt, cls = _multi_inputs(i, g.S, A, g.output_size // A)
        lib.rnn_amd_set_multi_step(g.handle, rc.iptr(hot), rc.iptr(nxt), rc.iptr(cls), A, MULTI_LEAKAGE, method, momentum)
    else:
        raise KeyError(site)


def oracle_step(site, o, text, i, method, momentum, batch=1):
    if site in ("char_step", "deltas_apply", "pernet"):
        o.char_step(text, i, method, momentum)
    elif site == "calculate":
        c = C.c_int(0)
        o.orc.orc_advance(o.z, 0)
        o.orc.orc_net_error_bptt(o.z, 0, int(text[i]), int(text[i + 1]), C.byref(c))
        o.orc.orc_bptt_calculate(o.z, 0, batch, momentum)
    elif site == "multi":
        A = o.input_size
        NC = o.output_size // A
        hot, nxt, cls = _multi_inputs(i, o.S, A, NC)
        ranges = (C.c_int * (2 * (NC + 1)))()
        for j in range(o.S):
            o.orc.orc_advance(o.z, j)
            o.orc.orc_multi_softmax_error(o.z, j, int(hot[j]), int(nxt[j]), int(cls[j]), A, MULTI_LEAKAGE, ranges)
            o.orc.orc_calc_deltas(o.z, j, 1 if j else 0, ranges)
        o.orc.orc_apply_learning(o.z, method, momentum)
    else:
        raise KeyError(site)


def full_kw(kw, method):
    kw = dict(kw)
    kw.setdefault("learn_rate", 1e-5)
    kw.setdefault("seed", 3)
    if method in NEEDS_AUX:
        kw["flags"] = AUX_FLAGS
    return kw


def prepare_oracle(o, method):
    a = o.arrays()
    if method == rc.ADAGRAD:
        for k in ("ih_m", "ho_m", "b_m"):
            if k in a:
                a[k][:] = BALLAST
    if method == rc.RPROP:
        a["ih_aux"][:] = AUX_START
        a["ho_aux"][:] = AUX_START


def prepare_device(lib, g, method):
    if method == rc.ADAGRAD:
        lib.rnn_set_momentum_values(g.net, BALLAST)
    if method == rc.RPROP:
        lib.rnn_set_aux_values(g.net, AUX_START)


def device_snapshot(g):
    """ApiSet.snapshot plus what the second-accumulator rules and the sparse top path keep"""
    snap = g.snapshot()
    n0 = g.net.contents
    b0 = n0.bptt.contents
    if n0.flags & rc.FLAG_AUX_ARRAYS:
        snap["ih_aux"] = rc.view(b0.ih_aux, g.I, g.H).copy()
        snap["ho_aux"] = rc.view(b0.ho_aux, g.H, g.O).copy()
        if g.bottom_inputs:
            bl = n0.bottom_layer.contents
            snap["b_aux"] = rc.view(bl.aux, bl.i_size, bl.o_size).copy()
    snap["err_a"] = np.stack([rc.view(g.nets[j].contents.bptt.contents.h_error, g.I).copy() for j in range(g.S)])
    return snap


def oracle_snapshot(o):
    snap = o.snapshot()
    a = o.arrays()
    for k in ("ih_aux", "ho_aux", "b_aux"):
        if k in a:
            snap[k] = a[k].copy()
    return snap


STATE_KEYS = ("ih_w", "ho_w", "ih_m", "ho_m", "ih_aux", "ho_aux", "ih_delta", "ho_delta", "hist", "hidden", "output",
              "o_error", "err_a", "index", "min_error_factor", "generation", "b_w", "b_m", "b_aux", "b_delta", "b_o_error")


def load_oracle(o, snap):
    """an oracle that continues from the state in `snap` (a device's or another oracle's), generators included"""
    a = o.arrays()
    for k in STATE_KEYS:
        if k in snap and k in a:
            a[k][:] = snap[k]
    for j in range(o.S):
        r = o.z.contents.rng[j]
        r.a, r.b, r.c, r.d = (int(x) for x in snap["rng"][j])


def load_device(lib, g, snap):
    """the device set continues from the state in `snap`: as test_gpu_parity.py's _load_state, and the ring index and
    the generation counter (both host-authoritative) with it, so that one state can be gone back to"""
    n0 = g.net.contents
    b0 = n0.bptt.contents

    def put():
        rc.view(n0.ih_weights, g.I, g.H)[:] = snap["ih_w"]
        rc.view(n0.ho_weights, g.H, g.O)[:] = snap["ho_w"]
        rc.view(b0.ih_momentum, g.I, g.H)[:] = snap["ih_m"]
        rc.view(b0.ho_momentum, g.H, g.O)[:] = snap["ho_m"]
    put()
    lib.rnn_amd_sync_host(g.net, rc.RNN_AMD_EVERYTHING)
    put()
    for j in range(g.S):
        n = g.nets[j].contents
        b = n.bptt.contents
        rc.view(b.history, g.D, g.I)[:] = snap["hist"][:, j, :]
        rc.view(n.hidden_layer, g.H)[:] = snap["hidden"][j]
        b.min_error_factor = float(snap["min_error_factor"][j])
        b.index = int(snap["index"][j])
        n.generation = int(snap["generation"][j])
    lib.rnn_amd_host_written(g.net, rc.RNN_AMD_EVERYTHING)
    if hasattr(g, "handle"):
        # the upload itself happens in the next set call, with the streams' learn_rate of THAT moment: a loss call (its
        # error vectors are the next generation's to overwrite) carries it out now, so that a rate written after this
        # has only push_learn_rates to reach the device by
        lib.rnn_amd_set_softmax_error(g.handle, rc.iptr(np.zeros(g.S, np.int32)))


def check_keys(site, method, kw):
    keys = list(KEYS)
    if kw.get("bottom_inputs"):
        keys += BOTTOM_KEYS
    if method in NEEDS_AUX:
        keys += ["ih_aux", "ho_aux"]
    if method == rc.RPROP:
        # RPROP steps by the SIGN of a delta: against another summation order a delta within rounding of zero flips a
        # step (test_gpu_dist.py leaves the oracle out for the same reason).  Its weights, previous
        # gradients and step sizes are held to the rule's restatement from the device's own deltas instead
        # (check_update_identity), which reads the same scalars.
        keys = [k for k in keys if k not in ("ih_w", "ho_w", "ih_m", "ho_m", "ih_aux", "ho_aux", "b_w", "b_m")]
    return keys


def elem_floor_of(kw):
    return 1e-1 if kw["learn_rate"] >= 0.05 else 1e-2   # (the hot regime's floor: replay.check)


# --------------------------------------------------------------------------------------- Part A: moved between calls --

class Pair:
    """one device set and one oracle at the same site"""

    def __init__(self, lib, site, kw, method, batch=1):
        self.lib, self.site, self.method, self.batch = lib, site, method, batch
        self.kw = kw = full_kw(kw, method)
        self.text = _case_text(site, kw)
        if site in ("pernet", "calculate"):
            self.g = sc.ApiSet(lib, softmax_best_guess=rc.load_oracle().orc_softmax_best_guess, **kw)
        else:
            self.g = sc.AmdBatchedSet(lib, **kw)
        self.o = sc.OracleSet(**kw)
        prepare_device(lib, self.g, method)
        prepare_oracle(self.o, method)
        self.state = {"momentum": 0.95}
        self.i = 0
        # small sets warm up in lock step, so that what no snapshot carries (the bottom layer's carry, stale entries
        # the sparse top path reads) is the oracle's own to rounding; at the large text shapes the oracle's generations
        # are the test's cost and nothing of that kind exists
        lockstep = kw["hidden_size"] <= 256
        for _ in range(kw["D"] + 3):
            self.dev(self.i)
            if lockstep:
                self.orc(self.i)
            self.i += 1

    def dev(self, i):
        device_step(self.site, self.lib, self.g, self.text, i, self.method, self.state["momentum"], self.batch)

    def orc(self, i):
        oracle_step(self.site, self.o, self.text, i, self.method, self.state["momentum"], self.batch)

    def write(self, scalar, value):
        write_scalar(scalar, value, self.g, self.o, self.state)

    def one_generation(self, label="", identity=False):
        """ONE generation on both sides from the device's state, compared.  A generation in which a pre-activation
        within rounding of zero takes another mask is not a parity case (test_gpu_parity.py's
        _one_generation_from_device_state): the next one is taken instead, under the same bounds, ONCE.  The bounds: every
        flipped value within 1e-5 of zero, and at most 10 per million hidden values -- a RATE, which a set of fewer than
        100,000 hidden values cannot show in one generation: there a single flip, the smallest event there is, is let
        through, and the rate is held over all the values the module compared (COUNTS: its last test)."""
        g, o = self.g, self.o
        COUNTS["comparisons"] += 1
        stats = hasattr(g, "handle") and self.site in ("char_step", "deltas_apply")
        for attempt in range(2):
            before = device_snapshot(g)
            load_oracle(o, before)
            if stats:
                g.stats(clear=True)
            self.dev(self.i)
            self.orc(self.i)
            self.i += 1
            sg, so = device_snapshot(g), oracle_snapshot(o)
            flipped = (sg["hidden"] != 0) != (so["hidden"] != 0)
            COUNTS["values"] += int(flipped.size)
            COUNTS["flipped"] += int(flipped.sum())
            if not flipped.any():
                break
            assert 1e6 * flipped.sum() / flipped.size <= 10.0 or flipped.sum() == 1, (
                "%s: %d of %d hidden values differ in being zero" % (label, flipped.sum(), flipped.size))
            assert np.abs(np.where(sg["hidden"][flipped] != 0, sg["hidden"][flipped], so["hidden"][flipped])).max() < 1e-5, label
            assert attempt == 0, "%s: a rounding-level mask flip in two generations running" % label
            COUNTS["retried"] += 1
        if stats and self.site == "char_step":
            got = g.stats().bptt_depth_sum
            assert got == float(so["bptt_depth"].sum()), "%s: bptt_depth_sum %g on the device, the oracle's depths %s" % (
                label, got, so["bptt_depth"].tolist())
        # Part A and, where asked for, Part B: both are evaluated, so that a failure names every check that saw it
        bad = []
        try:
            replay.check(sg, so, RTOL, keys=check_keys(self.site, self.method, self.kw),
                         exact=("index", "generation", "rng"), elem_floor=elem_floor_of(self.kw))
        except AssertionError as e:
            bad.append("against the oracle: %s" % e)
        if identity or self.method == rc.RPROP:
            try:
                self.identity(before, sg, label)
            except AssertionError as e:
                bad.append("against the rule's restatement: %s" % e)
        assert not bad, "%s: %s" % (label, " | ".join(bad))
        return before, sg, so

    def identity(self, before, after, label):
        z = self.o.z.contents
        lr = np.float32(self.o.arrays()["learn_rate"][0])
        rates = {"ih": lr, "ho": lr * np.float32(z.ho_scale), "b": lr * np.float32(z.b_learn_rate_scale)}
        check_update_identity(before, after, self.method, rates, self.state["momentum"], z.momentum_weight, self.kw)

    def close(self):
        self.g.close()
        self.o.close()


def run_moves(lib, site, kw, method, scalars, batch=1, identity=False, setup=None):
    """Part A's protocol for a chain of scalars on one set: warm up with the creation values; then per scalar a first
    move, a second move to another value, and the creation value again, one compared generation after each.  With
    `identity`, the first generation after each first move is also held to the rule's restatement (Part B)."""
    p = Pair(lib, site, kw, method, batch)
    try:
        if setup:
            setup(p)
        for scalar in scalars:
            for n, value in enumerate(moves(scalar, p.kw)):
                p.write(scalar, value)
                label = "%s %s move %d" % (site, scalar, n)
                p.one_generation(label, identity=identity and n == 0)
    finally:
        p.close()


# ------------------------------------------------------------------------- the guard: does the oracle see the move? --

_WARM = {}


def oracle_pair_differs(site, kw, method, scalar, batch=1, second=False):
    """Two oracles from ONE warmed-up state, one generation with the scalar's new value and one with the old:
    what a device with a stale scalar would look like to replay.check.  Returns the assertion's text, or None."""
    kw = full_kw(kw, method)
    key = (site, method, batch, json.dumps(kw, sort_keys=True))
    text = _case_text(site, kw)
    n = kw["D"] + 3
    if key not in _WARM:
        o = sc.OracleSet(**kw)
        prepare_oracle(o, method)
        for i in range(n):
            oracle_step(site, o, text, i, method, 0.95, batch)
        _WARM[key] = oracle_snapshot(o)
        o.close()
    snap = _WARM[key]
    vals = moves(scalar, kw)
    old, new = (vals[0], vals[1]) if second else (vals[2], vals[0])
    out = []
    for value in (new, old):
        o = sc.OracleSet(**kw)
        load_oracle(o, snap)
        st = {"momentum": 0.95}
        write_scalar(scalar, value, None, o, st)
        oracle_step(site, o, text, n, method, st["momentum"], batch)
        out.append(oracle_snapshot(o))
        o.close()
    keys = check_keys(site, method, kw)
    if method == rc.RPROP:
        keys = keys + ["ih_w", "ho_w", "ih_aux", "ho_aux"]   # (oracle against oracle: one summation order)
    try:
        replay.check(out[0], out[1], RTOL, keys=keys, exact=("index", "generation", "rng"), elem_floor=elem_floor_of(kw))
    except AssertionError as e:
        return str(e)
    return None


# ------------------------------------------------------------------------ Part B: the update, element by element --

EPS = 2.0 ** -24


def rule(method, w, m, aux, d, rate, momentum, mw):
    """The seven rules of rnn_apply_learning (recur-nn.c:454-593) in float64 from float32 operands, and per element a
    bound on what float32 arithmetic may differ from it by: every float32 operation adds at most 2^-24 of its result,
    divide and square root are allowed twice that; the bound is (operations on the path) x 2^-24 x (sum of the
    magnitudes of the terms added), times 2 for the order of operations.  fma contraction only removes roundings.
    Returns (w, m, aux) after and the three bounds."""
    f8 = np.float64
    w, m, d = f8(w), f8(m), f8(d)
    aux = None if aux is None else f8(aux)
    rate, momentum, mw = f8(np.float32(rate)), f8(np.float32(momentum)), f8(np.float32(mw))
    zero = np.zeros_like(w)
    if method in (rc.WEIGHTED, rc.SIMPLIFIED_NESTEROV, rc.CLASSICAL):
        if method == rc.SIMPLIFIED_NESTEROV:
            mw = f8(np.float32(momentum / (1.0 + momentum)))
        elif method == rc.CLASSICAL:
            mw = f8(1.0)
        t = d * rate
        w2 = w + (t + m * mw)                                    # mul, mul, add, add
        m2 = (m + t) * momentum                                  # mul, add, mul
        return (w2, m2, aux, 2 * 4 * EPS * (np.abs(w) + np.abs(t) + np.abs(m * mw)),
                2 * 3 * EPS * (np.abs(m) + np.abs(t)) * abs(momentum), zero)
    if method == rc.NESTEROV:
        t = d * rate
        m2 = (m + t) * momentum                                  # mul, add, mul
        w2 = (w + t) + m2                                        # ... and two adds
        return (w2, m2, aux, 2 * 5 * EPS * (np.abs(w) + np.abs(t) + np.abs(m2)),
                2 * 3 * EPS * (np.abs(m) + np.abs(t)) * abs(momentum), zero)
    if method == rc.ADAGRAD:
        a = m + d * d                                            # mul, add
        with np.errstate(invalid="ignore", divide="ignore"):
            step = d * rate / np.sqrt(a)                         # mul; sqrt and divide (two each) on a's two
        w2 = w + step                                            # add
        return w2, a, aux, 2 * 8 * EPS * (np.abs(w) + np.abs(step)), 2 * 2 * EPS * (np.abs(m) + d * d), zero
    if method == rc.ADADELTA:
        decay = momentum
        renewal = f8(np.float32(1.0) - np.float32(momentum))     # (a float32 subtraction in the rule)
        g = m * decay + (np.abs(d) * renewal + rate)             # mul, mul, add, add: all terms positive
        step = aux * decay / g * d                               # mul, divide (2), mul on g's four
        s = aux * decay + (np.abs(step) * renewal + rate)        # step's eight, mul, add, add and aux's mul
        w2 = w + step
        return w2, g, s, 2 * 9 * EPS * (np.abs(w) + np.abs(step)), 2 * 4 * EPS * np.abs(g), 2 * 12 * EPS * np.abs(s)
    if method == rc.RPROP:
        # branch predicates and clamps in float32, so that a product that underflows decides the same way
        f4 = np.float32
        d4, p4, s4, r4 = f4(d), f4(m), f4(aux), f4(rate)
        max_step, min_step = r4, f4(1e-6 * f8(r4))
        with np.errstate(under="ignore"):
            prod = d4 * p4
        step = np.where(prod > 0, np.minimum(s4 * f4(1.2), max_step),
                        np.where(prod < 0, np.maximum(s4 * f4(0.5), min_step), s4))
        d4 = np.where(prod < 0, f4(0), d4)
        w2 = np.where(d4 > 0, w + f8(step), w - f8(step))
        # the step: one multiplication and a clamp whose bound may be formed in float32 or float64; the weight: one add
        return w2, f8(d4), f8(step), 2 * 3 * EPS * (np.abs(w) + np.abs(step)), zero, 2 * 2 * EPS * np.abs(step)
    raise KeyError(method)


def trained_masks(snap, kw):
    """True where an element of W_ih / W_ho (/ the bottom layer's weights) ever receives a delta: not column 0 of W_ih
    (the bias unit has no input weights), not the columns above hidden_size, not the padding rows and columns"""
    hs, isz, osz = kw["hidden_size"], kw["input_size"], kw["output_size"]
    ih = np.zeros(snap["ih_w"].shape, bool)
    ih[:1 + hs + isz, 1:1 + hs] = True
    ho = np.zeros(snap["ho_w"].shape, bool)
    ho[:1 + hs, :osz] = True
    masks = {"ih": ih, "ho": ho}
    if "b_w" in snap:
        b = np.zeros(snap["b_w"].shape, bool)
        b[:1 + kw["bottom_inputs"], :isz] = True
        masks["b"] = b
    return masks


def check_update_identity(before, after, method, rates, momentum, mw, kw, label=""):
    """after.w, .m, .aux == rule(before.w, .m, .aux, the deltas the device stored, the caller's scalars), element by
    element within the rule's own rounding bound; elements that never train keep their weight's bits (under RPROP,
    which alone moves a weight whose delta is zero, the restatement's value) and have no delta."""
    masks = trained_masks(before, kw)
    bad = []
    for seg, (wk, mk, ak, dk) in (("ho", ("ho_w", "ho_m", "ho_aux", "ho_delta")), ("ih", ("ih_w", "ih_m", "ih_aux", "ih_delta")),
                                  ("b", ("b_w", "b_m", "b_aux", "b_delta"))):
        if wk not in before:
            continue
        aux = before[ak] if method in NEEDS_AUX else None
        w2, m2, a2, bw, bm, ba = rule(method, before[wk], before[mk], aux, after[dk], rates[seg], momentum, mw)
        for got, want, bound, name in ((after[wk], w2, bw, wk), (after[mk], m2, bm, mk)) + (
                ((after[ak], a2, ba, ak),) if aux is not None else ()):
            err = np.abs(np.float64(got) - want)
            over = ~(err <= bound)
            if over.any():
                i = np.unravel_index(np.argmax(np.where(over, np.nan_to_num(err - bound, nan=np.inf), -1)), err.shape)
                bad.append("%s: %d of %d elements beyond the rule's bound, worst at %s: got %.9g, want %.9g, bound %.3g" % (
                    name, over.sum(), over.size, i, got[i], want[i], bound[i]))
        idle = ~masks[seg]
        if np.abs(after[dk][idle]).max(initial=0.0) != 0:
            bad.append("%s: a delta where nothing trains" % dk)
        if method != rc.RPROP:
            if not np.array_equal(np.float32(w2)[idle], before[wk][idle]):
                bad.append("%s: the restatement moves weights that never train" % wk)
            if not np.array_equal(after[wk][idle].view(np.uint32), before[wk][idle].view(np.uint32)):
                bad.append("%s: weights that never train changed" % wk)
    assert not bad, "%s: %s" % (label, "; ".join(bad))


# ------------------------------------------------------------------------------------------- cases in a subprocess --

def run_in_subprocess(env_extra, spec, timeout=900):
    """cases under switches the library reads once (a process of their own); their counts are added to COUNTS"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(spec)], capture_output=True, text=True,
                       env=env, timeout=timeout, cwd=here)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    for k in COUNTS:
        COUNTS[k] += res[k]
    return res


def fast_paths_off_env():
    env = {}
    here = os.path.dirname(os.path.abspath(__file__))
    for line in open(os.path.join(here, "..", "tools", "all_fast_paths_off.env")):
        if line.strip() and not line.startswith("#"):
            k, v = line.strip().split("=")
            env[k] = v
    return env


def _join_one_rank(p):
    """the exchange step with one rank (RECUR_AMD_DIST_ONE_RANK_EXCHANGE=1 keeps it in): rnn_amd_set_char_step then goes
    deltas -> rnn_amd_set_apply_exchange, the sharded optimiser (k_apply_xchg) with rates of its own"""
    assert os.environ.get("RECUR_AMD_DIST_ONE_RANK_EXCHANGE") == "1"
    p.blob = C.create_string_buffer(rc.RNN_AMD_EXCHANGE_BLOB_BYTES)
    p.lib.rnn_amd_set_exchange_export(p.g.handle, p.blob)
    assert p.lib.rnn_amd_set_exchange_join(p.g.handle, 0, 1, p.blob, None, 1) == 0


def _worker(spec):
    lib = rc.load_amd()
    assert lib.rnn_amd_device_count() >= 1, "no HIP device: the product has no CPU fallback"
    for case in spec["cases"]:
        run_moves(lib, case.get("site", "char_step"), case["kw"], case["method"], case["scalars"],
                  identity=case.get("identity", False), setup=_join_one_rank if spec.get("exchange") else None)
    print("RESULT " + json.dumps(COUNTS))


if __name__ == "__main__":
    _worker(json.loads(sys.argv[1]))
