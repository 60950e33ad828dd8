"""What the tests of gstclassify's trainer on the device share (rnn_amd_set_classify_steps, rnn_amd_classify_generations;
maybe_learn, gstclassify.c:2180-2257): the numpy restatement of recur_amd/csrc/classify_train_rule.h, the cases, the loop of
rnn_amd_classify_generation the block call is held to, and the oracle twin -- maybe_learn written out over the oracle's
per-stream calls with the reference's `if (err_sum)`, as tests/test_gpu_callers.py has it for one generation.

The restatement takes `broken`, one rule broken at a time (BROKEN): tests/test_classify_train_rule.py shows that each broken
form differs from the whole one on the inputs used, so a device that ran the broken rule would be noticed."""
import ctypes as C
import ctypes.util

import numpy as np

import recur_ctypes as rc

F = np.float32
PARITY_BAR = 1e-4        # the project's parity bar (tests/test_gpu_callers.py: RTOL)
MOMENTUM = 0.9
SOFT_START = 2000.0      # gstclassify's default
BROKEN = ("active_on_any_non_negative", "gate_on_trained", "generation_for_inactive", "draws_group_major")


# ------------------------------------------------------------------ the rule, restated --

def np_trains(targets, gsize, broken=None):
    """[...][G] bool: the (stream, group) pairs that carry a label"""
    tg = np.asarray(targets)
    if broken == "active_on_any_non_negative":
        return tg >= 0
    return (tg >= 0) & (tg < np.asarray(gsize))


def np_decisions(targets, gsize, generation=None, broken=None):
    """targets [T][n][G] -> (masks uint8 [T][stride] with stride = n rounded up to 4 and zero padding, active int [T],
    generation counters uint32 [n] after the block)"""
    tg = np.asarray(targets, np.int32)
    T, n, _ = tg.shape
    stride = (n + 3) & ~3
    act = np_trains(tg, gsize, broken).any(axis=2)
    masks = np.zeros((T, stride), np.uint8)
    masks[:, :n] = act
    gen = np.zeros(n, np.uint32) if generation is None else np.array(generation, np.uint32)
    steps = np.full(n, T, np.uint32) if broken == "generation_for_inactive" else act.sum(axis=0).astype(np.uint32)
    return masks, act.sum(axis=1).astype(np.int64), gen + steps


def np_gate_raises(wrong, trained=True, broken=None):
    """a stream's summed wrongness raises the gate iff it is not 0.0f (NaN does, -0 does not)"""
    if broken == "gate_on_trained":
        return bool(trained)
    return bool(F(wrong) != F(0))


GATE_VALUES = (("zero", 0.0, 0), ("minus zero", -0.0, 0), ("smallest denormal", float(np.nextafter(F(0), F(1))), 1),
               ("negative denormal", -1e-40, 1), ("smallest normal", float(np.finfo(F).tiny), 1), ("one", 1.0, 1),
               ("infinity", float("inf"), 1), ("minus infinity", float("-inf"), 1), ("NaN", float("nan"), 1))

# (name, (have_features, have_targets, n_steps, ld, input_size, n_groups, offsets or None, sizes or None, output_size), code)
_OK = (1, 1, 2, 8, 8, 2, (0, 4), (3, 4), 8)


def _refusal(**change):
    keys = ("have_features", "have_targets", "n_steps", "ld", "input_size", "n_groups", "offsets", "sizes", "output_size")
    d = dict(zip(keys, _OK))
    d.update(change)
    return tuple(d[k] for k in keys)


REFUSALS = (
    ("valid", _refusal(), 0), ("valid: wider rows", _refusal(ld=11), 0), ("valid: one step", _refusal(n_steps=1), 0),
    ("valid: a group ends with the outputs", _refusal(offsets=(0, 4), sizes=(4, 4)), 0),
    ("no features", _refusal(have_features=0), 1), ("no targets", _refusal(have_targets=0), 1),
    ("no steps", _refusal(n_steps=0), 2), ("negative steps", _refusal(n_steps=-2), 2),
    ("rows one short", _refusal(ld=7), 3),
    ("no groups", _refusal(n_groups=0), 4), ("no offsets", _refusal(offsets=None), 4), ("no sizes", _refusal(sizes=None), 4),
    ("negative offset", _refusal(offsets=(-1, 4)), 5), ("empty group", _refusal(sizes=(3, 0)), 5),
    ("a group past the outputs", _refusal(sizes=(3, 5)), 5), ("offset 2^31 - 1", _refusal(offsets=(0, 2 ** 31 - 1)), 5),
)


class Jenkins:
    """recur-rng.h's generator (Bob Jenkins' small PRNG) from its four words"""
    M = (1 << 64) - 1

    def __init__(self, a, b, c, d):
        self.s = [int(a), int(b), int(c), int(d)]

    @staticmethod
    def _rot(x, k):
        return ((x << k) | (x >> (64 - k))) & Jenkins.M

    def rand64(self):
        a, b, c, d = self.s
        e = (a - self._rot(b, 7)) & self.M
        a = b ^ self._rot(c, 13)
        b = (c + self._rot(d, 37)) & self.M
        c = (d + e) & self.M
        d = (e + a) & self.M
        self.s = [a, b, c, d]
        return d


TO_UNIT = F(1.0) / F(float(0xfffffffffffffffe))


def np_unit_draw(bits64):
    return F(F(int(bits64)) * TO_UNIT)


_LIBM = C.CDLL(ctypes.util.find_library("m"))
_LIBM.powf.restype, _LIBM.powf.argtypes = C.c_float, [C.c_float, C.c_float]


def np_train_p(seen, bias):
    """(the power is the C library's powf, as the reference's: numpy's own float32 power is another function, an ulp off
    in places)"""
    seen = np.asarray(seen, np.uint32)
    share = F(1.0) / F(F(int(seen.sum()) & 0xffffffff) + F(1.0))
    base = (F(1.0) - seen.astype(F) * share).astype(F)
    return np.array([_LIBM.powf(float(b), float(F(bias))) for b in base], F)


def np_choose(targets, goff, gsize, train_p, seen, used, draws, broken=None):
    """one generation's balanced choice: targets [n][G] -> (use [n][G] with -1 where the pair does not train, trains [n],
    the draws consumed); seen and used are counted in place; draws: an iterator of 64-bit integers"""
    tg = np.asarray(targets, np.int32)
    n, G = tg.shape
    use = np.full((n, G), -1, np.int32)
    order = [(ch, g) for ch in range(n) for g in range(G)]
    if broken == "draws_group_major":
        order = [(ch, g) for g in range(G) for ch in range(n)]
    taken = 0
    for ch, g in order:
        t = int(tg[ch, g])
        if not 0 <= t < int(gsize[g]):
            continue
        out = int(goff[g]) + t
        seen[out] += 1
        taken += 1
        if train_p[out] > np_unit_draw(next(draws)):
            used[out] += 1
            use[ch, g] = t
    return use, (use >= 0).any(axis=1).astype(np.uint8), taken


# ------------------------------------------------------------------ the cases --

ONE_OF_2 = (np.array([0], np.int32), np.array([2], np.int32), 2)               # gstclassify's default: "01"
GAP = (np.array([0, 4], np.int32), np.array([3, 4], np.int32), 8)             # column 3 belongs to no group
WIDE = (np.array([0, 35], np.int32), np.array([30, 35], np.int32), 70)        # o_size 72: past the one-launch top


def block_of(T, n, n_in, groups, seed, ld=None, unlabelled=0.2, silent=()):
    """-> features float32 [T][n][ld], targets int32 [T][n][G]: a fifth of the pairs without a label (-1, or the group's
    size: both are "no label"); the generations in `silent` carry no label at all"""
    goff, gsize, _ = groups
    rs = np.random.default_rng([seed, T, n])
    ld = ld or n_in
    x = np.zeros((T, n, ld), F)
    x[:, :, :n_in] = (rs.standard_normal((T, n, n_in)) * 0.5).astype(F)
    x[:, :, n_in:] = 7.0          # (what lies between the rows is not an input)
    tg = np.stack([rs.integers(0, s, (T, n)) for s in gsize], axis=2).astype(np.int32)
    none = rs.random(tg.shape) < unlabelled
    tg[none] = np.where(rs.random(int(none.sum())) < 0.5, -1, np.broadcast_to(gsize, tg.shape)[none])
    for t in silent:
        tg[t] = -1
    return x, tg


def designed_targets():
    """[T][n][G] on GAP's groups: every kind of row -- both labelled, one labelled, none, a label equal to the size, one
    past it, INT_MIN -- and a generation without any label"""
    gs = GAP[1]
    rows = [(0, 0), (2, 3), (-1, 1), (1, -1), (-1, -1), (int(gs[0]), 0), (0, int(gs[1])), (int(gs[0]), int(gs[1])),
            (int(gs[0]) + 1, -7), (-2 ** 31, 2 ** 31 - 1), (2, -2 ** 31)]
    t0 = np.array(rows, np.int32)
    return np.stack([t0, np.roll(t0, 3, axis=0), np.full_like(t0, -1), t0[::-1]])


# ------------------------------------------------------------------ the loop the block call is held to --

def run_loop(lib, gs, x, tg, groups, weight=None, style=rc.NESTEROV, soft=SOFT_START, balance=None):
    """today's loop on an AmdBatchedSet: rnn_amd_classify_generation per window with exact_gate 1 -> groups trained"""
    goff, gsize, _ = groups
    w = None if weight is None else rc.fptr(np.ascontiguousarray(weight, F))
    trained = 0
    for t in range(x.shape[0]):
        xt, tt = np.ascontiguousarray(x[t]), np.ascontiguousarray(tg[t])
        trained += lib.rnn_amd_classify_generation(gs.handle, rc.fptr(xt), xt.shape[1], len(goff), rc.iptr(goff), rc.iptr(gsize),
                                                   rc.iptr(tt), w, balance, style, soft, 1)
    return trained


# ------------------------------------------------------------------ the oracle twin --

def oracle_generation(o, x, tg, groups, weight=None, style=rc.NESTEROV, momentum=MOMENTUM, soft=SOFT_START, flags=None,
                      gate="reference", n_in=None, likelihoods=None):
    """maybe_learn on an OracleSet: orc_clear_deltas; per channel orc_opinion, orc_grouped_softmax_error, orc_calc_deltas
    where a group was trained, orc_advance; `if (wrong)` orc_apply_learning with the soft-started momentum; orc_condition
    when flags is given.  gate "always": the update whenever a group trained (what exact_gate 0 does).  likelihoods: a list
    that takes every channel's softmax likelihoods of this generation (oracle_likelihoods' row), in channel order.
    -> (groups trained, the summed wrongness, each channel's wrongness float32 [S] (NaN where not trained), updated,
    the groups whose winner was the target)"""
    orc, z = o.orc, o.z
    goff, gsize, _ = groups
    w = None if weight is None else rc.fptr(np.ascontiguousarray(weight, F))
    n_in = n_in or o.input_size
    orc.orc_clear_deltas(z)
    wins, wrong, trained = C.c_int(0), C.c_float(0), 0
    each = np.full(o.S, np.nan, F)
    for j in range(o.S):
        orc.orc_opinion(z, j, rc.fptr(np.ascontiguousarray(x[j, :n_in])), 0.0)
        before = F(wrong.value)
        if likelihoods is not None:
            likelihoods.append(oracle_likelihoods(o, groups, [j])[0])
        k = orc.orc_grouped_softmax_error(z, j, len(goff), rc.iptr(goff), rc.iptr(gsize), rc.iptr(np.ascontiguousarray(tg[j])),
                                          w, C.byref(wins), C.byref(wrong))
        if k:
            orc.orc_calc_deltas(z, j, 1, None)
            each[j] = F(wrong.value) - before      # (exact where the sum so far is 0, which is where it is asked)
        trained += k
        orc.orc_advance(z, j)
    updated = bool(wrong.value) if gate == "reference" else trained > 0
    if updated:
        gen0 = float(o.arrays()["generation"][0])
        orc.orc_apply_learning(z, style, orc.orc_momentum_soft_start(gen0, momentum, soft))
    if flags is not None:
        orc.orc_condition(z, flags)
    return trained, float(wrong.value), each, updated, int(wins.value)


def oracle_likelihoods(o, groups, streams=None):
    """the softmax likelihoods of every group of the streams (all of them by default) from the oracle's outputs, by the
    oracle's own softmax: float32 [streams][sum of the sizes]"""
    goff, gsize, _ = groups
    out = o.arrays()["output"]
    like = []
    for j in (range(o.S) if streams is None else streams):
        row = []
        for a, s in zip(goff, gsize):
            src = np.ascontiguousarray(out[j, a:a + s], F)
            dst = np.zeros(int(s), F)
            o.orc.orc_softmax(rc.fptr(dst), rc.fptr(src), int(s))
            row.append(dst)
        like.append(np.concatenate(row))
    return np.array(like, F)


# ------------------------------------------------------------------ the gate script --
# A net whose output rows are written: the top layer's bias row holds +40 under class 0 and -40 under class 1 on top of the
# initialised weights, a logit gap of about 80.  The softmax likelihood of class 0 is then exactly 1.0f, so a generation
# whose labels are all class 0 has a summed wrongness of exactly 0: the reference makes no update (the gate stays closed),
# where "update whenever a group trained" would move the weights by the momentum arrays, which are written to non-zero.
# A label of class 1 has wrongness 1.  The rate is tiny, so the open generations leave the gap where it is.

GATE = dict(n_in=6, hidden=24, n=5, D=3, seed=23, learn_rate=1e-6, gap=40.0, momentum_value=2.0 ** -12)
GATE_LARGE = dict(GATE, n_in=32, hidden=512, n=128, D=12)      # the delta call leaves planes: k_apply's plane-summing branch
GATE_SCRIPT = ("open", "closed", "unlabelled", "open", "closed")
GATE_WANT = (True, False, False, True, False)                  # the updates of the script


def gate_kw(c=GATE):
    return dict(input_size=c["n_in"], hidden_size=c["hidden"], output_size=2, S=c["n"], D=c["D"], seed=c["seed"],
                learn_rate=c["learn_rate"], momentum=MOMENTUM)


def gate_net(ih_w, ho_w, c=GATE):
    """the written arrays from the initialised ones -> (ih_w, ho_w, ih_m, ho_m)"""
    ho = np.array(ho_w, F)
    ho[0, 0] += F(c["gap"])
    ho[0, 1] -= F(c["gap"])
    sign = np.where((np.indices(ih_w.shape).sum(axis=0) % 2) == 0, 1, -1)
    hid = c["hidden"]       # (the real weights only: column 0 is the bias unit, the columns past hidden_size are padding)
    ih_m = np.zeros_like(np.asarray(ih_w, F))
    ih_m[:1 + c["n_in"] + hid, 1:1 + hid] = (sign * c["momentum_value"]).astype(F)[:1 + c["n_in"] + hid, 1:1 + hid]
    ho_m = np.zeros_like(ho)
    ho_m[:1 + hid, :2] = F(c["momentum_value"])
    return np.array(ih_w, F), ho, ih_m, ho_m


def gate_block(c=GATE):
    """the script's features and targets: open = every second channel hears class 1, closed = class 0 or no label"""
    rs = np.random.default_rng([c["seed"], 5])
    T, n = len(GATE_SCRIPT), c["n"]
    x = (rs.standard_normal((T, n, c["n_in"])) * 0.5).astype(F)
    tg = np.zeros((T, n, 1), np.int32)
    for t, kind in enumerate(GATE_SCRIPT):
        if kind == "open":
            tg[t, :, 0] = np.arange(n) % 2
        elif kind == "closed":
            tg[t, :, 0] = np.where(np.arange(n) % 3 == 2, -1, 0)
        else:
            tg[t] = -1
    return x, tg


# ------------------------------------------------------------------ the oracle-comparison cases --
# (name, hidden, channels, depth, groups, seed).  tests/test_classify_train_cases_cpu.py shows from the oracle alone that
# no trained group of these has its two best likelihoods closer than the parity bar can move them: `correct` is then the
# same count on the device.

PARITY_CASES = (("one group of 2", 24, 5, 3, ONE_OF_2, 31), ("two groups with a gap", 99, 7, 4, GAP, 32),
                ("70 outputs", 24, 4, 3, WIDE, 33))
PARITY_T = 3
PARITY_N_IN = 10


def parity_kw(case):
    name, hidden, n, D, groups, seed = case
    return dict(input_size=PARITY_N_IN, hidden_size=hidden, output_size=groups[2], S=n, D=D, seed=seed, learn_rate=1e-3,
                momentum=MOMENTUM)


def parity_block(case, k=0):
    name, hidden, n, D, groups, seed = case
    return block_of(PARITY_T, n, PARITY_N_IN, groups, [seed, k])


def unclear_winners(like, tg, groups, bar=PARITY_BAR):
    """how many trained groups have their two best likelihoods within 2 * bar of the larger: a device within the bar of
    the oracle could pick the other one"""
    goff, gsize, _ = groups
    unclear, at = 0, 0
    for g, s in enumerate(gsize):
        p = np.sort(like[:, at:at + s], axis=1)
        at += int(s)
        if s < 2:
            continue
        trained = (tg[:, g] >= 0) & (tg[:, g] < s)
        unclear += int((trained & (p[:, -1] - p[:, -2] <= 2 * bar * p[:, -1])).sum())
    return unclear
