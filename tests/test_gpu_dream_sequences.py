"""Parrot's player on the device (rnn_amd_dream_sequences; recur_amd/csrc/dream_api.c, dream_rule.h, k_dream_step and
k_dream_draw in kernels_rows.hip) against the oracle and against the loop it replaces.

THE ORACLE is an OracleSet with one stream per sequence, the product's weights copied in (both get the same seeded numpy
weights), every stream starting from the product net's hidden row or from its h_in row, and a generator per sequence
(orc_init_rand64 of its seed).  The comparison is teacher-forced, as the automaton's and the sampler's: for frame t the
oracle's clone k is fed the row that the DEVICE's frame t - 1 and the oracle's own generator give by dream_next in numpy
float32 (dream_cases.py; `first` for t = 0); its hidden row is its own.  That row, behind the last frame, must be the
device's `next` bit for bit, and the oracle's generators the device's rng_out bit for bit.  dream_tanh of the oracle's raw
answer is held to the device's frame at the project's parity bar, and h_out to the oracle's hidden rows at the same bar
(test_gpu_trace_texts.at_the_bar, per sequence).

THE BAR ON A FRAME.  The bar is stated for what the forward pass computes, here the raw answers r of a sequence: the
2-norm and the largest difference within 1e-4 of the array's, an element that is not small (|r| >= 1e-2 R, R the array's
largest |r|) within 1e-4 of itself, a small one within 1e-4 * 1e-2 * R.  The device hands back tanh of its answers, not
the answers.  The tanh's slope is at most 1, and so is its logarithmic slope x sech^2 x / tanh x: an absolute error passes
through it no larger, and so does a relative one.  So the frame is held, element by element, to 1e-4 of dream_tanh(r)
where r is not small and to 1e-4 * 1e-2 * R where it is -- R being the largest |r| of the sequence's RAW answers over
the run, as at_the_bar takes it of a sequence's answers array, which the tanh has compressed to at most 1 while it left
the small elements as they were (frames_at_the_bar).  The bar's 2-norm and largest-difference
figures follow from the two element-wise ones on the raw row and do not carry through the compression: they are not asked
of the frame again.

UNCLEAR ELEMENTS: dream_tanh jumps from the fraction's 0.99990 to 1 at |x| = 4.97, so an element whose oracle |raw| lies
within 1e-4 * R + 1e-6 of 4.97 (R the row's largest |raw|: the bar's reach) may take either branch; it is held to the
branch the device took.  The unmarked tests assert, from the oracle's own closed-loop run alone, that every case keeps such
elements under 1 % and that its frames stay alive; the designed `hot` net's answers all pass the clamp (its frames are
exactly +-1.0f), the `warm` one's are a mixture.

AGAINST TODAY'S LOOP the check is bit for bit: per frame the same rows go through rnn_amd_run_sequences (n_groups == 0, one
frame each, states in place), dream_tanh and dream_next are applied by the host harness (dream_rule_harness.cpp, with the
oracle's generator), and frames, next, states and generators must equal the one call's -- at equal row counts, which
fwd_plan.h goes by.  Where two calls must agree they agree bit for bit as well: the same call twice, the segment size,
seeds against generators built from them, NULL against explicit start states, a run cut in two and joined in place, a
permuted batch.

The oracle's runs are computed once per case and shared."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import recur_ctypes as rc
import scenarios as sc
from dream_cases import (EXTREME, F, build_harness, from_words, gaussians, generator, harness_rows, np_fraction, np_next,
                         np_tanh, same_floats, words)
from recur_amd.drivers import dream_sequences, run_sequences
from test_gpu_trace_texts import BAR, FLOOR, at_the_bar

gpu = pytest.mark.gpu
CAP = 0.01
_cases = {}
_free = {}
_forced = {}
_nets = {}


class Case:
    """a net of `feats` inputs and outputs (seeded numpy weights, a seeded hidden row, half of it zeros as a rectifier
    leaves it), `rows` sequences with a first row and a seed each.  hot: the top layer's bias row is +-50, alternating:
    every answer passes the clamp.  clip: the first rows lie beyond the emergency soft clip of an input row"""

    def __init__(self, name, feats, hidden, rows, frames, seed, activation=rc.RELU, noise=1.0, top=1.5, hot=False, clip=False):
        self.name, self.feats, self.hidden, self.rows, self.frames = name, feats, hidden, rows, frames
        self.activation, self.noise, self.hot = activation, noise, hot
        g = np.random.default_rng(seed)
        sizes = [C.c_int(0) for _ in range(3)]
        rc.load_oracle().orc_padded_sizes(feats, hidden, feats, *[C.byref(x) for x in sizes])
        self.I, self.H, self.O = [x.value for x in sizes]
        self.ih = np.zeros((self.I, self.H), F)
        self.ho = np.zeros((self.H, self.O), F)
        # bias row 0.1, recurrent rows 1 / sqrt(hidden), input rows 1 / sqrt(feats) (an input is a tanh times 1 + noise);
        # W_ho is top / sqrt(hidden): top 1.5 gives answers of the order of 1, where the tanh bends and is not clamped
        self.ih[0, 1:1 + hidden] = 0.1 * g.standard_normal(hidden)
        self.ih[1:1 + hidden, 1:1 + hidden] = g.standard_normal((hidden, hidden)) / np.sqrt(hidden)
        self.ih[1 + hidden:1 + hidden + feats, 1:1 + hidden] = g.standard_normal((feats, hidden)) / np.sqrt(feats)
        self.ho[:1 + hidden, :feats] = g.standard_normal((1 + hidden, feats)) * (top / np.sqrt(hidden))
        if hot:
            self.ho[0, :feats] = np.where(np.arange(feats) % 2 == 0, 50.0, -50.0)
        self.row = self.state(g)
        self.first = (g.standard_normal((rows, feats)) * 0.5).astype(F)
        if clip:
            self.first = g.uniform(30.0, 50.0, (rows, feats)).astype(F)
            assert np.all(self.first.sum(axis=1) > 16.0 * self.I)   # (recur-nn.c:68-81: the row's sum against 16 a column)
        self.seeds = (np.arange(rows, dtype=np.uint64) * np.uint64(7919) + np.uint64(seed * 1000 + 1))

    def state(self, g):
        h = np.zeros(self.H, F)
        h[0] = 1.0
        h[1:1 + self.hidden] = np.maximum(g.standard_normal(self.hidden), 0.0) * 0.5
        return h


def case(name):
    if name not in _cases:
        made = {
            # feature counts at hidden 99: one, odd, a wave, past a wave, parrot's 256, past one stride of the workgroup
            "f1": lambda: Case(name, 1, 99, 5, 3, 41),
            "f3": lambda: Case(name, 3, 99, 5, 3, 42),
            "f64": lambda: Case(name, 64, 99, 5, 3, 43),
            "f65": lambda: Case(name, 65, 99, 5, 3, 44),
            "f256": lambda: Case(name, 256, 99, 5, 3, 45),
            "f257": lambda: Case(name, 257, 99, 5, 3, 46),
            # row counts at hidden 32: around a wave of the plan, around the scratch rows' 256, parrot's most
            "r1": lambda: Case(name, 8, 32, 1, 3, 51),
            "r63": lambda: Case(name, 8, 32, 63, 2, 52),
            "r64": lambda: Case(name, 8, 32, 64, 2, 53),
            "r65": lambda: Case(name, 8, 32, 65, 2, 54),
            "r256": lambda: Case(name, 8, 32, 256, 2, 55),
            "r257": lambda: Case(name, 8, 32, 257, 2, 56),
            "r2000": lambda: Case(name, 8, 32, 2000, 2, 57),
            "h1024": lambda: Case(name, 256, 1024, 64, 8, 58),
            "resqrt": lambda: Case(name, 64, 99, 5, 3, 61, activation=rc.RESQRT),
            "reclip20": lambda: Case(name, 64, 99, 5, 3, 62, activation=rc.RECLIP20),
            "nine": lambda: Case(name, 12, 32, 7, 9, 63),
            "quiet": lambda: Case(name, 12, 32, 7, 9, 63, noise=0.0),
            "quarter": lambda: Case(name, 12, 32, 7, 9, 63, noise=0.25),
            "hot": lambda: Case(name, 12, 32, 7, 3, 64, hot=True),
            "warm": lambda: Case(name, 64, 32, 7, 3, 65, top=8.0),
            "clip": lambda: Case(name, 64, 32, 5, 3, 66, clip=True),
        }
        _cases[name] = made[name]()
    return _cases[name]


FEATURES = ["f1", "f3", "f64", "f65", "f256", "f257"]
ROWS = ["r1", "r63", "r64", "r65", "r256", "r257", "r2000"]
OTHERS = ["h1024", "resqrt", "reclip20", "nine", "quiet", "quarter", "hot", "warm", "clip"]
ALL = FEATURES + ROWS + OTHERS
LOOPED = FEATURES + ["r1", "r63", "r64", "r65", "r256", "resqrt", "reclip20", "nine", "quiet", "quarter", "hot", "clip"]


class Judged:
    """one oracle frame: the raw answers [rows][feats], dream_tanh of them, and per element whether the bar's reach
    (1e-4 of the row's largest |raw|, and 1e-6) leaves its side of the clamp open"""

    def __init__(self, raw):
        self.raw = raw.copy()
        self.frame = np_tanh(raw)
        self.R = np.abs(raw).max(axis=1, keepdims=True).astype(np.float64)
        self.unclear = np.abs(np.abs(raw.astype(np.float64)) - float(EXTREME)) <= 1e-4 * self.R + 1e-6


def oracle_run(c, forced=None, h_in=None, frames=None, first=None, rng_in=None, noise=None):
    """the oracle's run of a case: free-running (forced None: a clone is fed what dream_next makes of its own frame) or
    teacher-forced (forced: the device's frames [n][rows][feats]).  Returns (the list of Judged frames, the rows behind
    the last frame [rows][feats], the final hidden rows [rows][H], the generators afterwards [rows][4])"""
    n = c.frames if frames is None else frames
    noise = c.noise if noise is None else noise
    o = sc.OracleSet(input_size=c.feats, hidden_size=c.hidden, output_size=c.feats, S=c.rows, D=1, activation=c.activation,
                     learn_rate=1e-3, seed=1)
    assert (o.I, o.H, o.O) == (c.I, c.H, c.O)
    arr = o.arrays()
    arr["ih_w"][:] = c.ih
    arr["ho_w"][:] = c.ho
    arr["hidden"][:] = h_in if h_in is not None else c.row[None, :]
    gens = [generator(int(s)) for s in c.seeds] if rng_in is None else [from_words(w) for w in rng_in]
    x = np.ascontiguousarray(c.first if first is None else first, F).copy()
    judged = []
    for t in range(n):
        for k in range(c.rows):
            o.orc.orc_opinion(o.z, k, rc.fptr(x[k]), 0.0)
        j = Judged(arr["output"][:, :c.feats])
        judged.append(j)
        a = j.frame if forced is None else forced[t]
        if noise == 0.0:
            x = np.ascontiguousarray(a, F).copy()
        else:
            x = np.stack([np_next(a[k], noise, gaussians(gens[k], c.feats)) for k in range(c.rows)])
    hidden = arr["hidden"].copy()
    o.close()
    return judged, x, hidden, np.stack([words(g) for g in gens])


def free(name):
    if name not in _free:
        _free[name] = oracle_run(case(name))
    return _free[name]


# ------------------------------------------------------------------ the oracle alone: no device --

@pytest.mark.parametrize("name", ALL)
def test_the_chosen_nets_keep_the_unclear_elements_under_the_cap_and_stay_alive(name):
    c = case(name)
    judged, nxt, _, rng = free(name)
    unclear = sum(int(j.unclear.sum()) for j in judged)
    elements = c.rows * c.feats * c.frames
    clamped = sum(int((np.abs(j.raw) >= EXTREME).sum()) for j in judged)
    R = max(float(j.R.max()) for j in judged)
    print("%s: %d elements, %d unclear (%.3f %%), %d beyond the clamp, largest |raw| %.3g"
          % (name, elements, unclear, 100.0 * unclear / elements, clamped, R))
    assert unclear <= CAP * elements
    assert all(np.all(np.isfinite(j.raw)) for j in judged)
    if c.hot:      # every answer passes the clamp: frames of exactly +-1.0f, both signs
        assert clamped == elements and all(sorted(np.unique(j.frame)) == [-1.0, 1.0] for j in judged)
        return
    if name == "warm":   # a mixture: both branches of the tanh, in every frame
        assert all(0.05 * j.raw.size < (np.abs(j.raw) >= EXTREME).sum() < 0.95 * j.raw.size for j in judged)
    if name not in ("warm", "clip"):
        assert clamped <= 0.05 * elements and R > 0.2    # where the tanh bends: few answers, if any, reach the clamp
    assert all(np.abs(j.raw).max() > 0.05 for j in judged)
    assert all(not np.array_equal(judged[t].frame, judged[t + 1].frame) for t in range(c.frames - 1))
    if c.noise == 0.0:
        assert same_floats(nxt, judged[-1].frame) and np.array_equal(rng, np.stack([words(generator(int(s))) for s in c.seeds]))
    else:
        assert not np.array_equal(nxt, judged[-1].frame)


def test_the_clip_cases_first_rows_are_clipped_and_no_other_cases_are():
    for name in ALL:
        c = case(name)
        total = 1.0 + c.row[1:].sum() + c.first.sum(axis=1)      # the input row's sum (recur-nn.c:68-81)
        assert np.all(total > 16.0 * c.I) if name == "clip" else np.all(total < 16.0 * c.I), name


# ------------------------------------------------------------------ the device --

@pytest.fixture(scope="module")
def amd():
    lib = rc.bind_char(rc.load_amd())
    assert lib.rnn_amd_device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return lib


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("dream_rule_gpu"))


def make_net(lib, c):
    net = lib.rnn_new(c.feats, c.hidden, c.feats, rc.FLAG_STANDARD, 1, None, 4, 1e-3, 0.9, 0.0, c.activation)
    n = net.contents
    assert (n.i_size, n.h_size, n.o_size) == (c.I, c.H, c.O)
    rc.view(n.ih_weights, c.I, c.H)[:] = c.ih
    rc.view(n.ho_weights, c.H, c.O)[:] = c.ho
    lib.rnn_amd_host_written(net, rc.RNN_AMD_WEIGHTS)
    lib.rnn_amd_sync_host(net, rc.RNN_AMD_STREAM)
    rc.view(n.hidden_layer, c.H)[:] = c.row
    lib.rnn_amd_host_written(net, rc.RNN_AMD_STREAM)
    return net


def product(lib, name):
    """the case's net in the product: made once and shared, never changed after this"""
    if name not in _nets:
        _nets[name] = make_net(lib, case(name))
    return _nets[name]


def snapshot(lib, net):
    """the net's hidden row, its generator and its weights, as the device has them"""
    lib.rnn_amd_sync_host(net, rc.RNN_AMD_EVERYTHING)
    n = net.contents
    return (rc.view(n.hidden_layer, n.h_size).copy(), (n.rng.a, n.rng.b, n.rng.c, n.rng.d),
            rc.view(n.ih_weights, n.i_size, n.h_size).copy(), rc.view(n.ho_weights, n.h_size, n.o_size).copy())


def run(lib, name, n_frames=None, first=None, **kw):
    """dream_sequences on the case's net, rows, seeds and noise, the net unchanged by the call"""
    c, net = case(name), product(lib, name)
    before = snapshot(lib, net)
    kw.setdefault("noise", c.noise)
    if "rng_in" not in kw and kw["noise"] != 0.0:
        kw.setdefault("seeds", c.seeds)
    got = dream_sequences(lib, net, c.first if first is None else first, c.frames if n_frames is None else n_frames, **kw)
    after = snapshot(lib, net)
    assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(before, after)), name
    return got


def forced(lib, name):
    """(the device's results for the case, the oracle teacher-forced with its frames), once per case"""
    if name not in _forced:
        got = run(lib, name)
        _forced[name] = (got, oracle_run(case(name), forced=got[0]))
    return _forced[name]


def frames_at_the_bar(got, want, raw, what):
    """a run's frames [n][rows][feats] against dream_tanh of the oracle's answers at the bar carried through the tanh (the
    module's docstring), per sequence over its whole answers array as at_the_bar is applied to a sequence's: element by
    element 1e-4 of the wanted value where the RAW answer is not small, 1e-4 * 1e-2 of the sequence's largest |raw| where
    it is"""
    g, w = got.astype(np.float64), want.astype(np.float64)
    d = np.abs(g - w)
    R = np.abs(raw).max(axis=(0, 2), keepdims=True).astype(np.float64)
    small = np.abs(raw) < FLOOR * R
    big_worst = (d[~small] / np.abs(w[~small])).max() if np.any(~small) else 0.0
    small_worst = (d / (FLOOR * R))[small].max() if np.any(small) else 0.0
    print("%s: %d elements, %d small; worst relative difference %.3g, worst small one %.3g of the largest"
          % (what, d.size, int(small.sum()), big_worst, small_worst * FLOOR))
    assert big_worst <= BAR and small_worst <= BAR, (what, big_worst, small_worst)


def held_to_the_oracle(c, got, oracle, what, noise=None):
    frames, nxt, h_out, rng = got
    judged, x, hidden, gens = oracle
    noise = c.noise if noise is None else noise
    assert frames.shape == (len(judged), c.rows, c.feats) and frames.dtype == F and not np.any(np.isnan(frames))
    unclear, wanted = 0, []
    for t, j in enumerate(judged):
        clamp_taken = np.abs(frames[t]) == 1.0
        wanted.append(np.where(j.unclear, np.where(clamp_taken, np.sign(j.raw).astype(F), np_fraction(j.raw)), j.frame).astype(F))
        unclear += int(j.unclear.sum())
    if judged:
        frames_at_the_bar(frames, np.stack(wanted), np.stack([j.raw for j in judged]), what)
    assert unclear <= CAP * frames.size, (what, unclear)
    assert same_floats(nxt, x), what                                  # the closed loop's row behind the last frame
    if noise == 0.0:
        assert same_floats(nxt, frames[-1])
    else:
        assert np.array_equal(rng, gens), what
    assert h_out.shape == (c.rows, c.H)
    for k in range(c.rows):
        at_the_bar(np.ascontiguousarray(h_out[k, 1:1 + c.hidden]), np.ascontiguousarray(hidden[k, 1:1 + c.hidden]),
                   "%s, state of sequence %d" % (what, k))


def same_bits(a, b, c):
    (fa, na, ha, ga), (fb, nb, hb, gb) = a, b
    return (np.array_equal(fa.view(np.uint32), fb.view(np.uint32)) and np.array_equal(na.view(np.uint32), nb.view(np.uint32))
            and np.array_equal(ha[:, 1:1 + c.hidden].view(np.uint32), hb[:, 1:1 + c.hidden].view(np.uint32))
            and np.array_equal(ga, gb))


# ------------------------------------------------------------------ 1. every case against the oracle --

@gpu
@pytest.mark.parametrize("name", ALL)
def test_frames_rows_states_and_generators_meet_the_oracle(amd, name):
    c = case(name)
    got, oracle = forced(amd, name)
    held_to_the_oracle(c, got, oracle, name)
    frames = got[0]
    if c.hot:
        assert sorted(np.unique(frames)) == [-1.0, 1.0]               # exactly +-1.0f
        assert np.array_equal(frames[0], np.tile(np.where(np.arange(c.feats) % 2 == 0, F(1.0), F(-1.0)), (c.rows, 1)))
    elif name == "warm":
        assert 0.05 < (np.abs(frames) == 1.0).mean() < 0.95
    else:
        assert np.abs(frames).max() > 0.05 and not np.array_equal(frames[0], frames[-1])


# ------------------------------------------------------------------ 2. against today's loop, bit for bit --

@gpu
@pytest.mark.parametrize("name", LOOPED)
def test_the_one_call_is_todays_per_frame_loop_bit_for_bit(amd, harness, tmp_path, name):
    """the recipe the call replaces: per frame rnn_amd_run_sequences on one-frame sequences with the states in place, then
    the rule on the host"""
    lib, c, net = amd, case(name), product(amd, name)
    got = forced(lib, name)[0]
    x = c.first.copy()
    rng = np.stack([words(generator(int(s))) for s in c.seeds])
    state, frames = None, []
    for t in range(c.frames):
        seqs = [x[k:k + 1] for k in range(c.rows)]
        if state is None:
            answers, state = run_sequences(lib, net, seqs, winners=False)            # from the net's hidden row
            state = np.ascontiguousarray(state)
        else:
            answers, _ = run_sequences(lib, net, seqs, h_in=state, in_place=True, winners=False)
        raw = np.concatenate([a for a, _ in answers])
        frame, x, rng = harness_rows(harness, tmp_path, c.noise, raw, rng)
        frames.append(frame)
    mine = (np.stack(frames), x, state, rng if c.noise != 0.0 else got[3])
    assert same_bits(got, mine, c), name


# ------------------------------------------------------------------ 3. calls that must agree, bit for bit --

@gpu
def test_the_same_call_twice(amd):
    for name in ("f257", "r65"):
        assert same_bits(run(amd, name), forced(amd, name)[0], case(name)), name


@gpu
def test_frame_counts_and_the_segment_size_change_no_bit(amd):
    c = case("nine")
    whole = forced(amd, "nine")[0]
    assert whole[0].shape[0] == 9
    for segment in (1, 4, 9, 1000):                       # 9 frames as 9 x 1, 4 + 4 + 1, one
        assert same_bits(run(amd, "nine", segment_frames=segment), whole, c), segment
    for n in (1, 2):                                      # a shorter run is the longer one's beginning
        frames, nxt, h_out, rng = run(amd, "nine", n_frames=n)
        assert np.array_equal(frames.view(np.uint32), whole[0][:n].view(np.uint32)), n
        held_to_the_oracle(c, (frames, nxt, h_out, rng), oracle_run(c, forced=frames, frames=n), "nine, %d frames" % n)
    for name in ("quiet", "quarter"):
        assert same_bits(run(amd, name, segment_frames=4), forced(amd, name)[0], case(name)), name


@gpu
def test_noise_levels(amd):
    """0 draws nothing, touches no generator and needs none; 1 and 0.25 differ from it and from one another"""
    quiet, loud, quarter = [forced(amd, name)[0] for name in ("quiet", "nine", "quarter")]
    assert np.array_equal(quiet[0][0], loud[0][0]) and np.array_equal(quiet[0][0], quarter[0][0])   # frame 0: nothing drawn yet
    assert not np.array_equal(quiet[0][1], loud[0][1]) and not np.array_equal(quarter[0][1], loud[0][1])
    assert same_floats(quiet[1], quiet[0][-1])                                   # next is the last frame
    assert np.array_equal(loud[3], quarter[3])                                   # the same draws, scaled
    c = case("quiet")
    given = np.stack([words(generator(int(s))) for s in c.seeds])
    with_seeds = run(amd, "quiet", seeds=c.seeds)
    with_rng = run(amd, "quiet", rng_in=given)
    assert np.array_equal(with_seeds[3], given) and np.array_equal(with_rng[3], given)   # as they started
    assert same_bits(with_seeds, with_rng, c) and np.array_equal(with_seeds[0], quiet[0])
    assert np.all(quiet[3] == 0)                                                 # (the driver's zeros: not written)


@gpu
def test_seeds_are_the_generators_built_from_them(amd):
    for name in ("nine", "f65"):
        c = case(name)
        given = np.stack([words(generator(int(s))) for s in c.seeds])
        assert same_bits(run(amd, name, rng_in=given), forced(amd, name)[0], c), name
        assert same_bits(run(amd, name, rng_in=given, seeds=c.seeds[::-1].copy()), forced(amd, name)[0], c), name   # rng_in goes first


@gpu
def test_null_states_are_the_nets_hidden_row(amd):
    for name in ("nine", "r257"):
        c = case(name)
        assert same_bits(run(amd, name, h_in=np.tile(c.row, (c.rows, 1))), forced(amd, name)[0], c), name


def own_states(c):
    g = np.random.default_rng(77)
    return np.stack([c.state(g) for _ in range(c.rows)])


@gpu
def test_a_run_cut_in_two_and_joined_in_place_is_the_uncut_run(amd):
    """9 frames against 4 + 5, joined through next -> first, the states and the generators updated where they lie"""
    for name in ("nine", "quarter", "quiet"):
        c = case(name)
        start = own_states(c)
        given = np.stack([words(generator(int(s))) for s in c.seeds])
        uncut = run(amd, name, h_in=start, rng_in=given)
        state, gens = start.copy(), given.copy()
        f1, n1, h1, g1 = run(amd, name, n_frames=4, h_in=state, rng_in=gens, in_place=True)
        assert np.shares_memory(h1, state) and np.shares_memory(g1, gens) and not np.array_equal(state, start)
        assert (c.noise == 0.0) == np.array_equal(gens, given)
        f2, n2, h2, g2 = run(amd, name, n_frames=5, first=n1, h_in=state, rng_in=gens, in_place=True)
        assert same_bits((np.concatenate([f1, f2]), n2, state, gens), uncut, c), name
        # and distinct start states meet the oracle as the shared one does
        held_to_the_oracle(c, uncut, oracle_run(c, forced=uncut[0], h_in=start), name + ", a start state per sequence")
        assert not np.array_equal(uncut[0], forced(amd, name)[0][0])
    # no frames: rows, states and generators come back as they went in
    frames, nxt, h_none, g_none = run(amd, "nine", n_frames=0, h_in=start, rng_in=given)
    c = case("nine")
    assert frames.shape == (0, c.rows, c.feats) and same_floats(nxt, c.first) and np.array_equal(g_none, given)
    assert np.array_equal(h_none[:, 1:1 + c.hidden], start[:, 1:1 + c.hidden])


@gpu
def test_a_permuted_batch_is_the_same_per_sequence(amd):
    for name in ("nine", "r65", "f257"):
        c = case(name)
        perm = np.random.default_rng(5).permutation(c.rows)
        start = own_states(c)
        straight = run(amd, name, h_in=start)
        frames, nxt, h_out, rng = run(amd, name, first=c.first[perm], seeds=c.seeds[perm], h_in=start[perm])
        back = np.argsort(perm)
        assert same_bits((frames[:, back], nxt[back], h_out[back], rng[back]), straight, c), name


@gpu
def test_rows_wider_than_the_inputs(amd):
    """ld_first > input_size: the floats behind a row's inputs are not read as inputs"""
    c = case("f65")
    wide = np.full((c.rows, c.feats + 3), np.nan, F)
    wide[:, :c.feats] = c.first
    assert same_bits(run(amd, "f65", first=wide), forced(amd, "f65")[0], c)


# ------------------------------------------------------------------ 4. the net is left alone --

@gpu
def test_the_net_computes_next_what_a_twin_that_made_no_call_computes(amd):
    """(run() asserts for every call that hidden row, generator and weights are unchanged on both sides)"""
    lib, c = amd, case("nine")
    caller, idle = make_net(lib, c), make_net(lib, c)
    got = dream_sequences(lib, caller, c.first, c.frames, noise=c.noise, seeds=c.seeds)
    assert same_bits(got, forced(lib, "nine")[0], c)
    answers = []
    for net in (caller, idle):
        out = lib.rnn_opinion(net, rc.fptr(c.first[3]), 0.0)
        answers.append(rc.view(out, c.O)[:c.feats].copy())
        lib.rnn_amd_sync_host(net, rc.RNN_AMD_STREAM)
        answers.append(rc.view(net.contents.hidden_layer, c.H)[1:1 + c.hidden].copy())
    assert np.array_equal(answers[0].view(np.uint32), answers[2].view(np.uint32))
    assert np.array_equal(answers[1].view(np.uint32), answers[3].view(np.uint32))
    assert np.any(answers[0] != 0.0)
    for net in (caller, idle):
        lib.rnn_delete_net(net)


# ------------------------------------------------------------------ 5. the tool --

@gpu
def test_the_tool_writes_the_drivers_bytes(amd, tmp_path):
    lib, c = amd, case("nine")
    path = str(tmp_path / "parrot.net")
    assert lib.rnn_save_net(product(lib, "nine"), path.encode(), 0) == 0 and os.path.exists(path)
    tool = os.path.join(rc.ROOT, "build", "parrot_dream_amd")
    for args, channels, n, seed, noise in ((["-c", "5", "-n", "4", "-s", "9"], 5, 4, 9, 1.0),
                                           (["-c", "3", "-n", "2", "-s", "11", "-z", "0.25"], 3, 2, 11, 0.25),
                                           (["-n", "3", "-z", "0"], 1, 3, 1, 0.0)):
        loaded = lib.rnn_load_net(path.encode())   # the tool starts from the state the file holds: so does the driver
        want = dream_sequences(lib, loaded, np.zeros((channels, c.feats), F), n, noise=noise,
                               seeds=np.arange(channels, dtype=np.uint64) + np.uint64(seed), want_out=False)[0]
        lib.rnn_delete_net(loaded)
        out = str(tmp_path / "frames.f32")
        r = subprocess.run([tool] + args + [path, out], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-2000:]
        got = np.fromfile(out, F)
        assert got.size == n * channels * c.feats and np.array_equal(got.view(np.uint32), want.ravel().view(np.uint32)), args
        assert len(np.unique(got)) > 8
    r = subprocess.run([tool, "-c", "0", path, str(tmp_path / "none.f32")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and not os.path.exists(str(tmp_path / "none.f32"))
