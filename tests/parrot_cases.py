"""What tests/test_parrot_rule.py, tests/test_parrot_cases_cpu.py and tests/test_gpu_parrot_training.py share: the numpy
float32 restatement of recur_amd/csrc/parrot_rule.h (gstparrot.c:464-477; the tanh is dream_cases.np_tanh), the shapes and
seeded inputs of the GPU cases, and the oracle twin of one generation of parrot's trainer.  The oracle has no tanh loss:
its twin writes the rule, in numpy float32, through OracleSet.arrays()'s writable `output` and `o_error` views between
orc_opinion and orc_calc_deltas.  numpy rounds every float32 operation once and fuses none, which is the rule."""
import os
import subprocess

import numpy as np

import dream_cases as dc
import recur_ctypes as rc
import scenarios as sc

F = np.float32
ROOT = rc.ROOT
SRC = os.path.join(ROOT, "tests", "parrot_rule_harness.cpp")
MOMENTUM = 0.95          # gstparrot.h: MOMENTUM, what maybe_learn hands to rnn_apply_learning
BROKEN = ("diff - a * a * diff", "(1 - a) * diff", "slope * (a - target)", "fused fmaf(-a, a, 1)")


def build_harness(directory, extra=()):
    exe = os.path.join(str(directory), "parrot_rule_harness" + ("_san" if extra else ""))
    subprocess.run(dc.CXX + list(extra) + [SRC, "-o", exe], check=True)
    return exe


def np_error(a, target, broken=None):
    """parrot_error: (1 - a * a) * (target - a), four roundings; and its broken forms"""
    a, t = np.asarray(a, F), np.asarray(target, F)
    with np.errstate(all="ignore"):
        diff = (t - a).astype(F)
        if broken == "diff - a * a * diff":
            return (diff - (a * a).astype(F) * diff).astype(F)
        if broken == "(1 - a) * diff":
            return ((F(1.0) - a) * diff).astype(F)
        if broken == "fused fmaf(-a, a, 1)":  # one rounding of 1 - a^2: float64 holds the square of a float32 exactly
            slope = (1.0 - a.astype(np.float64) * a.astype(np.float64)).astype(F)
            return (slope * diff).astype(F)
        slope = (F(1.0) - (a * a).astype(F)).astype(F)
        if broken == "slope * (a - target)":
            return (slope * (a - t).astype(F)).astype(F)
        assert broken is None, broken
        return (slope * diff).astype(F)


def np_loss(a, target):
    """parrot_loss: (target - a)^2, two roundings"""
    a, t = np.asarray(a, F), np.asarray(target, F)
    with np.errstate(all="ignore"):
        diff = (t - a).astype(F)
        return (diff * diff).astype(F)


def np_rule(raw, target):
    """-> (answer, error, loss) of raw outputs against their targets"""
    a = dc.np_tanh(raw)
    return a, np_error(a, target), np_loss(a, target)


def edge_pairs():
    """a in {0, +-denormal, +-1, the neighbours of +-1, NaN} x targets in {0, +-1, +-0.5, NaN}"""
    one = F(1.0)
    a = [F(0.0), F(-0.0), F(1e-45), F(-1e-45), F(1e-39), F(-1e-39), one, -one, np.nextafter(one, F(0)), np.nextafter(one, F(2)),
         np.nextafter(-one, F(0)), np.nextafter(-one, F(-2)), F(np.nan)]
    t = [F(0.0), one, -one, F(0.5), F(-0.5), F(np.nan)]
    aa, tt = np.meshgrid(np.array(a, F), np.array(t, F), indexing="ij")
    return aa.ravel().copy(), tt.ravel().copy()


def sweep_pairs(count=100000, seed=1234):
    """seeded (answer, target) pairs: answers as the tanh leaves them, targets in [-1, 1]"""
    rs = np.random.default_rng(seed)
    raw = (rs.standard_normal(count) * 2.0).astype(F)
    return dc.np_tanh(raw), rs.uniform(-1.0, 1.0, count).astype(F)


# ------------------------------------------------------------------ the GPU cases --

def _case(name, hidden, S, D, n_in, n_out, n=None, activation=rc.RELU, **more):
    c = dict(name=name, hidden=hidden, S=S, D=D, n_in=n_in, n_out=n_out, n=n_out if n is None else n, activation=activation,
             saturated=False)
    c.update(more)
    return c


# one generation from the device's state against the oracle (test_gpu_parrot_training.py, 2)
GENERATION_CASES = (
    # every wave boundary of the one-launch loss (thread x takes column x: waves 0 .. 3), o_size 4 .. 256
    [_case("outputs %d" % o, 64, 5, 3, 12, o) for o in (1, 4, 63, 64, 65, 255, 256)] +
    [_case("outputs 260: past the top launch", 64, 5, 3, 12, 260),
     # (flat weights of variance 2 / h_size answer beyond 4 at h_size 16: a narrower draw, test_parrot_cases_cpu.py)
     _case("hidden 12: fewer rows than waves", 12, 5, 3, 12, 8, variance=0.03),
     # (256 inputs in [-1, 1]: narrower draws again, so that the hidden sums and the answers stay of order 1)
     _case("parrot's default net", 199, 33, 4, 256, 256, variance=0.005),
     _case("hidden 1100: two passes of the backprop loop", 1100, 5, 3, 12, 64),
     _case("hidden 1024 resqrt", 1024, 32, 3, 256, 256, activation=rc.RESQRT, variance=0.001),
     _case("hidden 128 reclip20", 128, 32, 3, 256, 256, activation=rc.RECLIP20, variance=0.005),
     _case("n < output_size", 64, 5, 3, 12, 8, n=3)])
SATURATED_CASE = _case("saturated", 64, 5, 3, 12, 8, saturated=True)
SATURATED_BIAS = F(8.0)   # every raw answer is +-8: beyond the tanh's 4.97
FORMS = ("separate", "opinion_tanh_error", "dense_step")


def case_kw(c):
    kw = dict(input_size=c["n_in"], hidden_size=c["hidden"], output_size=c["n_out"], S=c["S"], D=c["D"],
              learn_rate=1e-5 if c["hidden"] > 1000 else 1e-3, seed=81, momentum=MOMENTUM, activation=c["activation"])
    if "variance" in c:
        kw["variance"] = c["variance"]
    return kw


def case_data(c, gen):
    """generation gen's rows: inputs [S][n_in] and targets [S][n] seeded uniform in [-1, 1], and for n < output_size the
    error planted behind column n (non-zero up to output_size, zero in the padding)"""
    rs = np.random.default_rng([GENERATION_CASES.index(c) if c in GENERATION_CASES else 99, gen])
    x = rs.uniform(-1.0, 1.0, (c["S"], c["n_in"])).astype(F)
    t = rs.uniform(-1.0, 1.0, (c["S"], c["n"])).astype(F)
    planted = None
    if c["n"] < c["n_out"]:
        planted = rs.uniform(0.05, 0.2, (c["S"], c["n_out"])).astype(F) * rs.choice([F(-1), F(1)], (c["S"], c["n_out"]))
        planted = planted.astype(F)
    return np.ascontiguousarray(x), np.ascontiguousarray(t), planted


def padded_error(planted, O):
    e = np.zeros((planted.shape[0], O), F)
    e[:, :planted.shape[1]] = planted
    return e


def saturated_ho(H, O, output_size):
    """the top layer of the saturated case: the bias row alone, +-SATURATED_BIAS in alternation"""
    ho = np.zeros((H, O), F)
    ho[0, :output_size] = SATURATED_BIAS * np.where(np.arange(output_size) % 2, F(-1), F(1))
    return ho


def oracle_generation(o, x, t, n, planted=None, momentum=MOMENTUM, advance=True, clear=True, accumulate=True, update=True):
    """one generation of parrot's trainer on an OracleSet: orc_clear_deltas; per stream orc_advance, orc_opinion, the rule
    through the writable views, orc_calc_deltas(z, j, 1, None); orc_apply_learning.  -> (raw answers [S][n], the loss terms
    [S][n] float32).  advance / clear / accumulate switch one of them off (accumulate False: the plugin's overwrite)."""
    orc, z = o.orc, o.z
    a = o.arrays()
    if clear:
        orc.orc_clear_deltas(z)
    raws, losses = np.zeros((o.S, n), F), np.zeros((o.S, n), F)
    for j in range(o.S):
        if advance:
            orc.orc_advance(z, j)
        orc.orc_opinion(z, j, rc.fptr(np.ascontiguousarray(x[j])), 0.0)
        if planted is not None:
            a["o_error"][j] = padded_error(planted, o.O)[j]
        raws[j] = a["output"][j, :n]
        ans, err, loss = np_rule(raws[j], t[j])
        a["output"][j, :n] = ans
        a["o_error"][j, :n] = err
        losses[j] = loss
        orc.orc_calc_deltas(z, j, 1 if accumulate else 0, None)
    if update:
        orc.orc_apply_learning(z, rc.WEIGHTED, momentum)
    return raws, losses


def free_running(c, generations):
    """the oracle alone through `generations` generations of case c from its seed -> (the OracleSet, raw answers per
    generation, loss terms per generation)"""
    o = sc.OracleSet(**case_kw(c))
    if c["saturated"]:
        o.arrays()["ho_w"][:] = saturated_ho(o.H, o.O, o.output_size)
    raws, losses = [], []
    for gen in range(generations):
        x, t, planted = case_data(c, gen)
        r, l = oracle_generation(o, x, t, c["n"], planted)
        raws.append(r)
        losses.append(l)
    return o, raws, losses


# ------------------------------------------------------------------ the learning case --
# two channels of 256 bins, each a travelling bump: frame t + 1 is frame t moved on by a fixed number of bins, which a
# net with a hidden layer learns to predict within a few hundred generations

LEARN = dict(channels=2, hidden=32, depth=8, rate=0.003, generations=400, block=50, seed=11)


def learning_frames(generations=None):
    """-> float32 [generations + 1][channels][256] within [-0.8, 0.8]"""
    T = (LEARN["generations"] if generations is None else generations) + 1
    bins = np.arange(256)
    fr = np.zeros((T, LEARN["channels"], 256), F)
    for ch in range(LEARN["channels"]):
        period, step = (16, 3) if ch == 0 else (32, 5)
        for t in range(T):
            fr[t, ch] = (0.8 * np.sin(2 * np.pi * (bins + step * t) / period)).astype(F)
    return fr
