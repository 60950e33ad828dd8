"""Many texts against one classifier net in one batched device run (rnn_amd_classify_texts; recur_amd/csrc/
classify_texts_api.c, classify_rule.h, k_classify_step in kernels_rows.hip) against the oracle: an OracleSet with one stream
per text, the product's weights copied in (both get the same seeded numpy weights), every stream starting from the product
net's hidden row or from its h_in row, then per symbol orc_one_hot_opinion with noise 0, orc_softmax over all outputs,
orc_softmax_best_guess and orc_capped_log2f -- the loop body of text-classify-results.c:96-104 and of
rnn_char_classify_epoch's validation (charmodel-classify.c:181-191) -- with the sums formed in float64.

THE BAR is the project's parity bar (test_gpu_trace_texts.at_the_bar: 1e-4 on the 2-norm and on the largest element,
element by element 1e-4 relative on the elements of at least 1e-2 of the array's largest, the bound of an element at that
floor below it), applied per text to its sums and to its sums of squares and per case to the texts' errors and entropies.
(at_the_bar takes float32 arrays: the doubles are rounded to float for it, 6e-8 of the bar's 1e-4.)  `count` is exact.
`correct` is TEACHER-CHECKED: a symbol whose two largest oracle probabilities lie within 1e-4 of the larger is unclear, and
a text's `correct` must lie in [clear hits, clear hits + unclear symbols].  That the chosen inputs keep the unclear symbols
at or under 1 % of a case's classed symbols, and that the cap case really underflows, is asserted from the oracle alone,
without a device (the unmarked tests).

Where two calls must agree they agree bit for bit: NULL against explicit start states, the final state of a cut joined by
h_out -> h_in in place, the caller's order.  The same row counts per pass launch the same kernels on the same rows.

The oracle's results are computed once per case and shared."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import loss_edge_cases as le
import recur_ctypes as rc
import scenarios as sc
from recur_amd.drivers import classify_texts, run_sequences
from test_gpu_trace_texts import BAR, at_the_bar, margins

gpu = pytest.mark.gpu
NO_CLASS = 0xFF
_cases = {}
_wants = {}
_nets = {}


class Case:
    """a net (seeded numpy weights, a seeded hidden row, half of it zeros as a rectifier leaves it) and a batch of texts
    with skips and class bytes; classed: "all", "half" (the even texts; the others have a NULL classes[k]) or None (classes
    is NULL); own_states: every text starts from a state of its own (h_in) instead of the net's hidden row"""

    def __init__(self, name, hidden, outputs, lens, seed, inputs=42, skips=None, classed="all", activation=rc.RELU,
                 feed=1.0, top=1.0, own_states=False, no_class=0.2):
        self.name, self.inputs, self.hidden, self.outputs = name, inputs, hidden, outputs
        self.lens, self.seed, self.activation, self.own_states = list(lens), seed, activation, own_states
        g = np.random.default_rng(seed)
        sizes = [C.c_int(0) for _ in range(3)]
        rc.load_oracle().orc_padded_sizes(inputs, hidden, outputs, *[C.byref(x) for x in sizes])
        self.I, self.H, self.O = [x.value for x in sizes]
        # test_gpu_texts_wide.seeded_net's weights, which test_gpu_run_sequences starts from: bias row 0.1, recurrent rows
        # 1 / sqrt(hidden), one-hot input rows `feed` (hidden values of about 1), W_ho top / sqrt(hidden)
        self.ih = np.zeros((self.I, self.H), np.float32)
        self.ho = np.zeros((self.H, self.O), np.float32)
        self.ih[0, 1:1 + hidden] = 0.1 * g.standard_normal(hidden)
        self.ih[1:1 + hidden, 1:1 + hidden] = g.standard_normal((hidden, hidden)) / np.sqrt(hidden)
        self.ih[1 + hidden:1 + hidden + inputs, 1:1 + hidden] = g.standard_normal((inputs, hidden)) * feed
        self.ho[:1 + hidden, :outputs] = g.standard_normal((1 + hidden, outputs)) * (top / np.sqrt(hidden))
        self.row = self.state(g)
        self.h_in = np.stack([self.state(g) for _ in self.lens]) if own_states else None
        self.texts = [g.integers(0, inputs, n).astype(np.uint8) for n in self.lens]
        self.skips = None if skips is None else list(skips)
        self.classes = None if classed is None else [self.class_bytes(g, n, no_class) if classed == "all" or k % 2 == 0 else None
                                                     for k, n in enumerate(self.lens)]

    def state(self, g):
        h = np.zeros(self.H, np.float32)
        h[0] = 1.0
        h[1:1 + self.hidden] = np.maximum(g.standard_normal(self.hidden), 0.0) * 0.5
        return h

    def class_bytes(self, g, n, no_class):
        cls = g.integers(0, min(self.outputs, 255), n).astype(np.uint8)
        cls[g.random(n) < no_class] = NO_CLASS
        return cls

    def skip(self, k):
        return max(self.skips[k], 0) if self.skips else 0


def cap_case(name):
    """a designed net (loss_edge_cases.designed_weights: symbol c's output row is written, whatever the state): symbol 0
    leaves class 0 eighty below class 1, p[0] = exp(-80) < 1e-30 -- the entropy of a symbol 0 of class 0 is the cap, 100;
    symbols 1 and 2 leave ordinary rows"""
    c = Case(name, 99, 5, [9, 4, 1, 6], 31, inputs=3, classed="all", no_class=0.0)
    rows = [np.array([0, 80, 0, 0, 0], np.float32), np.array([1, 0, -1, 0.5, 2], np.float32),
            np.array([-2, 0.25, 3, 1, 0], np.float32)]
    c.ih, c.ho = le.designed_weights(c.I, c.H, c.O, c.hidden, rows)
    c.texts = [np.array(t, np.uint8) for t in ([0, 1, 0, 2, 0, 0, 1, 2, 0], [1, 0, 2, 0], [0], [2, 1, 1, 2, 1, 2])]
    c.classes = [np.array(t, np.uint8) for t in ([0, 4, 0, 2, 1, 0, NO_CLASS, 2, 0], [4, 0, 2, 1], [0], [2, 4, 0, 2, 4, 3])]
    return c


# symbol counts that make the passes of one call run at 256, 192, 128, 64, 63 and 1 rows (test_gpu_texts_wide.LENS, a
# symbol less: every symbol has a pass here), and 4 texts more: a second wave
WIDE_LENS = [1] * 64 + [2] * 64 + [3] * 64 + [4] + [5] * 62 + [6] + [1] * 4
WIDE_ROWS = [256, 192, 128, 64, 63, 1]
BASE_LENS = [90, 0, 1, 2, 33, 90, 7, 0, 64, 65, 3, 12, 45, 1, 2, 71, 5, 18, 29, 8, 56, 4, 80, 10]
BASE_SKIPS = [0, 0, 0, 1, 3, 2, 7, 2, 1, 0, 3, 0, 2, 1, 0, 3, 9, 1, 0, 2, 3, 0, 1, 2]   # text 6: skip == len; 16: skip > len
COUNTS = [1, 2, 64, 65, 70, 200]
SMALL = [12, 5, 0, 9, 1]


def case(name):
    if name not in _cases:
        wide_lens = [int(x) for x in np.random.default_rng(3).permutation(WIDE_LENS)]
        made = {
            "base": lambda: Case(name, 99, 5, BASE_LENS, 11, skips=BASE_SKIPS, classed="half"),
            "unclassed": lambda: Case(name, 99, 5, BASE_LENS[:8], 11, skips=BASE_SKIPS[:8], classed=None),
            "states": lambda: Case(name, 99, 5, [20, 13, 20, 7, 1, 0, 16], 16, skips=[0, 2, 1, 0, 0, 0, 3], own_states=True),
            "wide": lambda: Case(name, 1024, 3, wide_lens, 17, skips=[k % 2 for k in range(len(wide_lens))]),
            "resqrt": lambda: Case(name, 99, 5, SMALL, 18, activation=rc.RESQRT),
            "reclip20": lambda: Case(name, 99, 5, SMALL, 19, activation=rc.RECLIP20, feed=30.0, top=0.1),
            "cap": lambda: cap_case(name),
        }
        for n in COUNTS:   # 1 and 2 classes; a wave exactly, one more, wider than a wave, and 200: lane-strided
            made["classes%d" % n] = lambda n=n: taught(Case(name, 99, n, SMALL, 20 + n))
        _cases[name] = made[name]()
    return _cases[name]


def taught(c):
    """among many classes a random class byte is hardly ever the best guess: every other symbol's class becomes the
    oracle's own pick, so that `correct` counts hits as well as misses"""
    p = oracle_run(c, c.texts, None, None, np.tile(c.row, (len(c.texts), 1))).p
    for cls, like in zip(c.classes, p):
        cls[::2] = np.argmax(like[::2], axis=1).astype(np.uint8) if len(cls) else cls[::2]
    return c


class Want:
    """the oracle's run of a case: sums, sumsqs [n][outputs] float64; error, entropy [n] float64; count, clear (hits among
    the clear symbols), unclear [n] int64; p: per text the probabilities [len][outputs] float32; h_out [n][H]"""


def oracle_run(c, texts, skips, classes, start):
    """texts through an OracleSet with c's weights from the states `start` [n][H]"""
    n = len(texts)
    o = sc.OracleSet(input_size=c.inputs, hidden_size=c.hidden, output_size=c.outputs, S=max(n, 1), D=1,
                     activation=c.activation, learn_rate=1e-3, seed=1)
    assert (o.I, o.H, o.O) == (c.I, c.H, c.O)
    arr = o.arrays()
    arr["ih_w"][:] = c.ih
    arr["ho_w"][:] = c.ho
    arr["hidden"][:n] = start
    w = Want()
    w.sums, w.sumsqs = np.zeros((n, c.outputs)), np.zeros((n, c.outputs))
    w.error, w.entropy = np.zeros(n), np.zeros(n)
    w.count, w.clear, w.unclear = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    w.p = []
    err = np.zeros(c.outputs, np.float32)
    for k, t in enumerate(texts):
        p = np.zeros((len(t), c.outputs), np.float32)
        skip = max(skips[k], 0) if skips else 0
        cls = classes[k] if classes is not None else None
        for j, symbol in enumerate(t):
            out = o.orc.orc_one_hot_opinion(o.z, k, int(symbol), 0.0)
            raw = np.ascontiguousarray(np.ctypeslib.as_array(out, shape=(o.O,))[:c.outputs])
            o.orc.orc_softmax(rc.fptr(p[j]), rc.fptr(raw), c.outputs)
            if j < skip:
                continue
            w.sums[k] += p[j].astype(np.float64)
            w.sumsqs[k] += (p[j] * p[j]).astype(np.float64)     # the product in float, the addition in double
            if cls is None or cls[j] == NO_CLASS:
                continue
            cl = int(cls[j])
            w.error[k] += 1.0 - float(p[j, cl])
            w.entropy[k] -= float(o.orc.orc_capped_log2f(float(p[j, cl])))
            w.count[k] += 1
            best = o.orc.orc_softmax_best_guess(rc.fptr(err), rc.fptr(raw), c.outputs)
            if c.outputs > 1 and margins(p[j])[1] <= BAR:
                w.unclear[k] += 1
            else:
                w.clear[k] += int(best == cl)
        w.p.append(p)
    w.h_out = arr["hidden"][:n].copy()
    o.close()
    return w


def want(name):
    if name not in _wants:
        c = case(name)
        start = c.h_in if c.own_states else np.tile(c.row, (len(c.texts), 1))
        _wants[name] = oracle_run(c, c.texts, c.skips, c.classes, start)
    return _wants[name]


ALL = ["base", "unclassed", "states", "wide", "resqrt", "reclip20", "cap"] + ["classes%d" % n for n in COUNTS]


# ------------------------------------------------------------------ the oracle alone: no device --

@pytest.mark.parametrize("name", ALL)
def test_the_chosen_inputs_keep_the_unclear_symbols_under_the_cap(name):
    c, w = case(name), want(name)
    classed = 0 if c.classes is None else sum(int((cls[c.skip(k):] != NO_CLASS).sum()) for k, cls in enumerate(c.classes)
                                              if cls is not None)
    print("%s: %d classed symbols, %d with the oracle's best within 1e-4 of the runner-up, %d clear hits"
          % (name, classed, w.unclear.sum(), w.clear.sum()))
    assert w.count.sum() == classed and w.unclear.sum() <= 0.01 * classed
    assert (classed > 0) == (name != "unclassed")
    for k, p in enumerate(w.p):     # a classifier's answers: the probabilities of every symbol add up to one
        assert np.allclose(p.sum(axis=1), 1.0, atol=1e-5)
        scored = max(len(p) - c.skip(k), 0)
        assert abs(w.sums[k].sum() - scored) <= 1e-5 * max(scored, 1)
    if c.outputs > 1 and name != "cap" and classed >= 15:   # neither always right nor always wrong
        assert 0 < w.clear.sum() < classed
    if name == "base":
        assert [n for n in c.lens if n < 3] == [0, 1, 2, 0, 1, 2] and max(c.lens) == 90
        assert c.skips[6] == c.lens[6] and c.skips[16] > c.lens[16] and not w.sums[6].any() and not w.sums[16].any()
        assert any(cls is None for cls in c.classes) and w.count.sum() < sum(len(cls) for cls in c.classes if cls is not None)
    if name == "reclip20":   # the activation's ceiling is met
        assert np.any(w.h_out[:, 1:1 + c.hidden] == 20.0)
    if name == "wide":       # the design: one call's passes at 256, 192, 128, 64, 63 and 1 rows, and a second wave
        first = sorted(c.lens, reverse=True)[:256]
        assert [sum(n > t for n in first) for t in range(max(first))] == WIDE_ROWS and len(c.lens) == 260


def test_the_cap_case_really_underflows():
    c, w = case("cap"), want("cap")
    capped = 0
    for k, (t, cls) in enumerate(zip(c.texts, c.classes)):
        for j in range(len(t)):
            if t[j] == 0 and cls[j] == 0:
                assert w.p[k][j, 0] < 1e-30
                capped += 1
            elif cls[j] != NO_CLASS:
                assert w.p[k][j, cls[j]] > 1e-3
    ordinary = np.array([sum(-np.log2(float(w.p[k][j, cls[j]])) for j in range(len(t)) if cls[j] != NO_CLASS
                             and not (t[j] == 0 and cls[j] == 0)) for k, (t, cls) in enumerate(zip(c.texts, c.classes))])
    per_text = np.array([sum(1 for j in range(len(t)) if t[j] == 0 and cls[j] == 0) for t, cls in zip(c.texts, c.classes)])
    print("cap: %d capped symbols, entropies %s" % (capped, w.entropy))
    assert capped == 6 and list(per_text) == [4, 1, 1, 0]
    assert np.allclose(w.entropy - ordinary, 100.0 * per_text, rtol=0, atol=1e-4)   # exactly 100 per such symbol


# ------------------------------------------------------------------ the device --

@pytest.fixture(scope="module")
def amd():
    lib = rc.bind_classify(rc.bind_char(rc.load_amd()))
    assert lib.rnn_amd_device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return lib


def product(lib, name):
    """the case's net in the product: made once and shared, never changed after this"""
    if name not in _nets:
        c = case(name)
        net = lib.rnn_new(c.inputs, c.hidden, c.outputs, rc.FLAG_STANDARD, 1, None, 4, 1e-3, 0.9, 0.0, c.activation)
        n = net.contents
        assert (n.i_size, n.h_size, n.o_size) == (c.I, c.H, c.O)
        rc.view(n.ih_weights, c.I, c.H)[:] = c.ih
        rc.view(n.ho_weights, c.H, c.O)[:] = c.ho
        lib.rnn_amd_host_written(net, rc.RNN_AMD_WEIGHTS)
        lib.rnn_amd_sync_host(net, rc.RNN_AMD_STREAM)
        rc.view(n.hidden_layer, c.H)[:] = c.row
        lib.rnn_amd_host_written(net, rc.RNN_AMD_STREAM)
        _nets[name] = net
    return _nets[name]


def snapshot(lib, net):
    """the net's hidden row, its generator and its weights, as the device has them"""
    lib.rnn_amd_sync_host(net, rc.RNN_AMD_EVERYTHING)
    n = net.contents
    return (rc.view(n.hidden_layer, n.h_size).copy(), (n.rng.a, n.rng.b, n.rng.c, n.rng.d),
            rc.view(n.ih_weights, n.i_size, n.h_size).copy(), rc.view(n.ho_weights, n.h_size, n.o_size).copy())


def untouched(before, after):
    return all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(before, after))


def run(lib, name, texts=None, **kw):
    """classify_texts on the case's net with its skips and classes (and its own start states), the net -- weights, hidden
    row and generator -- unchanged by the call"""
    c, net = case(name), product(lib, name)
    before = snapshot(lib, net)
    if texts is None:
        kw.setdefault("skips", c.skips)
        kw.setdefault("classes", c.classes)
    if c.own_states:
        kw.setdefault("h_in", c.h_in)
    got = classify_texts(lib, net, c.texts if texts is None else texts, **kw)
    assert untouched(before, snapshot(lib, net)), name
    return got


def f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def held_to_the_oracle(name, got, w=None, what=None):
    """sums, sums of squares, errors and entropies at the bar, counts exact, correct teacher-checked, h_out at the bar"""
    c, w, what = case(name), w or want(name), what or name
    sums, sumsqs, scores, h_out = got
    n = len(w.p)
    assert sums.shape == sumsqs.shape == (n, c.outputs) and scores.shape == (n,)
    worst = np.zeros(3)
    for k in range(n):
        worst = np.maximum(worst, at_the_bar(f32(sums[k]), f32(w.sums[k]), "%s, sums of text %d" % (what, k)))
        worst = np.maximum(worst, at_the_bar(f32(sumsqs[k]), f32(w.sumsqs[k]), "%s, sums of squares of text %d" % (what, k)))
    print("%s: error %s want %s" % (what, scores["error"], w.error))
    print("%s: entropy %s want %s" % (what, scores["entropy"], w.entropy))
    print("%s: correct %s clear %s unclear %s count %s" % (what, scores["correct"], w.clear, w.unclear, scores["count"]))
    worst = np.maximum(worst, at_the_bar(f32(scores["error"]), f32(w.error), what + ", errors"))
    worst = np.maximum(worst, at_the_bar(f32(scores["entropy"]), f32(w.entropy), what + ", entropies"))
    print("%s: %d texts, largest differences: 2-norm %.3g, largest element %.3g, element by element %.3g" % (what, n, *worst))
    assert np.array_equal(scores["count"], w.count)
    assert np.all(scores["correct"] >= w.clear) and np.all(scores["correct"] <= w.clear + w.unclear)
    if h_out is not None:
        assert h_out.shape == (n, c.H) and not np.any(np.isnan(h_out[:, 1:1 + c.hidden]))
        for k in range(n):
            at_the_bar(h_out[k, 1:1 + c.hidden], w.h_out[k, 1:1 + c.hidden], "%s, state %d" % (what, k))


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))


def states_equal(c, ha, hb):
    return np.array_equal(ha[:, 1:1 + c.hidden].view(np.uint32), hb[:, 1:1 + c.hidden].view(np.uint32))


def added(a, b):
    """the results of two chunks of the same texts as one: sums and scores add up, the states are the second's"""
    scores = a[2].copy()
    for field in ("error", "entropy", "correct", "count"):
        scores[field] = a[2][field] + b[2][field]
    return a[0] + b[0], a[1] + b[1], scores, b[3]


# ------------------------------------------------------------------ 1. the base case --

@gpu
def test_the_base_case(amd):
    """hidden 99, 42 inputs, 5 classes, 24 texts of 0, 1, 2 .. 90 symbols, skips of 0 .. 3, one equal to its text's length
    and one beyond it, class bytes on every other text with a fifth of them 0xFF, a NULL classes[k] on the others"""
    c, w = case("base"), want("base")
    got = run(amd, "base")   # (the driver asserts the guards behind every array and that every sum was written)
    held_to_the_oracle("base", got)
    sums, sumsqs, scores, h_out = got
    for k in (1, 7):         # the texts without a symbol: zeros, and their start state back -- the net's hidden row
        assert not sums[k].any() and not sumsqs[k].any() and scores[k]["count"] == 0
        assert np.array_equal(h_out[k, 1:1 + c.hidden], c.row[1:1 + c.hidden])
    for k in (6, 16):        # fed and never scored: zeros, and a state that has moved
        assert not sums[k].any() and scores[k]["count"] == 0
        assert not np.array_equal(h_out[k, 1:1 + c.hidden], c.row[1:1 + c.hidden])
    assert all(scores[k]["count"] == 0 and scores[k]["error"] == 0 for k in range(1, len(c.lens), 2))   # a NULL classes[k]
    assert scores["count"].sum() > 100
    # classes == NULL: the same sums to the bit, no score; skips == NULL scores every symbol; h_out may be left out
    bare = run(amd, "base", classes=None, want_out=False)
    assert bare[3] is None and np.array_equal(bare[0], sums) and np.array_equal(bare[1], sumsqs)
    assert not bare[2]["count"].any() and not bare[2]["error"].any() and not bare[2]["entropy"].any()
    every = run(amd, "base", skips=None)
    assert np.allclose(every[0].sum(axis=1), c.lens, rtol=1e-5) and states_equal(c, every[3], h_out)
    held_to_the_oracle("unclassed", run(amd, "unclassed"))


# ------------------------------------------------------------------ 2. the class count --

@gpu
@pytest.mark.parametrize("n", COUNTS)
def test_class_counts(amd, n):
    """1 class (every probability is 1) and 2; 64, a wave exactly, and 65; 70 and 200, lane-strided over the wave"""
    name = "classes%d" % n
    got = run(amd, name)
    held_to_the_oracle(name, got)
    if n == 1:
        c = case(name)
        assert np.array_equal(got[0][:, 0], np.array(c.lens, np.float64)) and np.array_equal(got[2]["correct"], got[2]["count"])
        assert not got[2]["error"].any() and not got[2]["entropy"].any()


# ------------------------------------------------------------------ 3. width, the other activations --

@gpu
def test_hidden_1024_at_every_row_count_and_a_second_wave(amd):
    """hidden 1024, 42 inputs, 3 classes; 260 texts whose symbol counts run one call's passes at 256, 192, 128, 64, 63 and 1
    rows, and a second wave of 4"""
    held_to_the_oracle("wide", run(amd, "wide"))


@gpu
@pytest.mark.parametrize("name", ["resqrt", "reclip20"])
def test_the_other_activations(amd, name):
    held_to_the_oracle(name, run(amd, name))


# ------------------------------------------------------------------ 4. states --

@gpu
def test_null_states_are_the_nets_hidden_row(amd):
    c = case("base")
    plain = run(amd, "base")
    filled = run(amd, "base", h_in=np.tile(c.row, (len(c.texts), 1)))
    assert same_bits(plain, filled) and states_equal(c, plain[3], filled[3])


@gpu
def test_a_cut_joined_through_the_states_in_place_is_the_uncut_call(amd):
    """texts of equal length cut at one place: both calls' passes run at the same row counts as the uncut call's, so the
    final state is the uncut call's to the bit; the counts are its counts; the sums differ by the grouping of their double
    additions alone"""
    c = case("states")
    g = np.random.default_rng(6)
    texts = [g.integers(0, c.inputs, 24).astype(np.uint8) for _ in range(5)]
    classes = [c.class_bytes(g, 24, 0.2) for _ in texts]
    skips = [0, 3, 12, 1, 24]
    start = np.stack([c.state(g) for _ in texts])
    uncut = run(amd, "states", texts, skips=skips, classes=classes, h_in=start)
    state = start.copy()
    first = run(amd, "states", [t[:10] for t in texts], skips=skips, classes=[x[:10] for x in classes], h_in=state, in_place=True)
    assert first[3] is not None and np.shares_memory(first[3], state) and not states_equal(c, state, start)
    second = run(amd, "states", [t[10:] for t in texts], skips=[max(s - 10, 0) for s in skips],
                 classes=[x[10:] for x in classes], h_in=state, in_place=True)
    joined = added(first, second)
    assert states_equal(c, state, uncut[3])
    assert np.array_equal(joined[2]["count"], uncut[2]["count"]) and np.array_equal(joined[2]["correct"], uncut[2]["correct"])
    assert uncut[2]["count"].sum() > 40
    for mine, whole in ((joined[0], uncut[0]), (joined[1], uncut[1]), (joined[2]["error"], uncut[2]["error"]),
                        (joined[2]["entropy"], uncut[2]["entropy"])):
        assert np.all(np.abs(mine - whole) <= 1e-12 * np.abs(whole)), np.abs(mine - whole).max()


@gpu
def test_distinct_start_states_and_ragged_chunks_meet_the_oracle(amd):
    c = case("states")
    got = run(amd, "states")
    held_to_the_oracle("states", got)
    assert np.array_equal(got[3][5, 1:1 + c.hidden], c.h_in[5, 1:1 + c.hidden])   # no symbol: the start state
    # every text cut at a place of its own, the second call from the first one's states
    cuts = [7, 13, 0, 3, 1, 0, 15]
    first = run(amd, "states", [t[:n] for t, n in zip(c.texts, cuts)], skips=c.skips,
                classes=[x[:n] for x, n in zip(c.classes, cuts)])
    second = run(amd, "states", [t[n:] for t, n in zip(c.texts, cuts)], skips=[max(s - n, 0) for s, n in zip(c.skips, cuts)],
                 classes=[x[n:] for x, n in zip(c.classes, cuts)], h_in=first[3])
    held_to_the_oracle("states", added(first, second), what="states, ragged chunks")


# ------------------------------------------------------------------ 5. the order does not matter --

@gpu
def test_a_permuted_batch_gives_the_permuted_results(amd):
    c = case("base")
    got = run(amd, "base")
    perm = [int(x) for x in np.random.default_rng(9).permutation(len(c.texts))]
    again = run(amd, "base", [c.texts[k] for k in perm], skips=[c.skips[k] for k in perm],
                classes=[c.classes[k] for k in perm])
    assert same_bits([x[perm] for x in got[:3]], again) and states_equal(c, again[3], got[3][perm])


# ------------------------------------------------------------------ 6. the cap --

@gpu
def test_the_entropy_grows_by_the_cap_where_the_probability_underflows(amd):
    c, w = case("cap"), want("cap")
    got = run(amd, "cap")
    held_to_the_oracle("cap", got)
    # without the capped symbols' classes the entropy is 100 per such symbol less, exactly as far as a double holds it
    classes = [np.where((t == 0) & (cls == 0), NO_CLASS, cls).astype(np.uint8) for t, cls in zip(c.texts, c.classes)]
    without = run(amd, "cap", c.texts, classes=classes)
    capped = got[2]["count"] - without[2]["count"]
    assert list(capped) == [4, 1, 1, 0]
    assert np.allclose(got[2]["entropy"] - without[2]["entropy"], 100.0 * capped, rtol=0, atol=1e-9)
    assert np.allclose(got[2]["error"] - without[2]["error"], 1.0 * capped, rtol=0, atol=1e-9)   # 1 - p, p below 1e-30


# ------------------------------------------------------------------ 7. today's route --

@gpu
def test_agreement_with_one_hot_rows_through_run_sequences(amd):
    """the same texts expanded on the host into one-hot rows, through rnn_amd_run_sequences with all outputs as one class
    group, its answers summed on the host in float64: the route this call replaces"""
    c, net = case("base"), product(amd, "base")
    sums, sumsqs, _, h_out = run(amd, "base", skips=None, classes=None)
    seqs = [np.eye(c.inputs, dtype=np.float32)[t] for t in c.texts]
    answers, h_seq = run_sequences(amd, net, seqs, groups=[(0, c.outputs)], winners=False)
    for k, (ans, _) in enumerate(answers):
        at_the_bar(f32(sums[k]), f32(ans.astype(np.float64).sum(axis=0)), "sums, text %d" % k)
        at_the_bar(f32(sumsqs[k]), f32((ans * ans).astype(np.float64).sum(axis=0)), "sums of squares, text %d" % k)
        at_the_bar(h_out[k, 1:1 + c.hidden], h_seq[k, 1:1 + c.hidden], "state %d" % k)


# ------------------------------------------------------------------ 8. the character layer and the tool --

@gpu
def test_the_character_layer_and_the_tool_print_what_the_driver_returns(amd, tmp_path):
    lib, c = amd, case("base")
    net = product(lib, "base")
    assert c.inputs == len(rc.DEFAULT_CHARSET)
    m = rc.CharMetadata(rc.DEFAULT_CHARSET, rc.DEFAULT_COLLAPSE_CHARS, False, True, True)
    p = lib.rnn_char_construct_metadata(C.byref(m))
    keep = C.create_string_buffer(C.string_at(p))
    C.CDLL(None).free(C.c_void_p(p))
    path = str(tmp_path / "classifier.net")
    net.contents.metadata = C.cast(keep, C.c_char_p)
    saved = lib.rnn_save_net(net, path.encode(), 0)
    net.contents.metadata = None
    assert saved == 0 and os.path.exists(path)
    raw = open(rc.EREWHON, "rb").read()
    pieces = [raw[20000:20400], raw[26000:26090], raw[31000:31002], raw[33000:33150]]
    names = []
    for k, piece in enumerate(pieces):
        names.append(str(tmp_path / ("part%d.txt" % k)))
        open(names[-1], "wb").write(piece)
    ignore = 3
    loaded = lib.rnn_load_net(path.encode())   # the tool starts from the state the file holds: so does the driver
    alphabet = lib.rnn_char_new_alphabet_from_net(loaded)
    texts = []
    for piece in pieces:
        n = C.c_int(0)
        q = lib.rnn_char_alloc_encoded_text(alphabet, piece, len(piece), C.byref(n), None, False)
        texts.append(np.ctypeslib.as_array(q, shape=(n.value,)).copy())
    assert [len(t) > ignore for t in texts] == [True, True, False, True] and all(len(t) for t in texts)
    sums, sumsqs, _, _ = classify_texts(lib, loaded, texts, skips=[ignore] * len(texts), want_out=False)
    mean, stddev = np.full((len(texts), c.outputs), np.nan), np.full((len(texts), c.outputs), np.nan)
    dp = C.POINTER(C.c_double)
    r = lib.rnn_amd_char_classify_texts(loaded, alphabet, (C.c_char_p * len(pieces))(*pieces),
                                        rc.iptr(np.array([len(x) for x in pieces], np.int32)), len(pieces), ignore,
                                        mean.ctypes.data_as(dp), stddev.ctypes.data_as(dp))
    assert r == 0
    lib.rnn_char_free_alphabet(alphabet)
    lib.rnn_delete_net(loaded)
    want_lines = []
    for k, t in enumerate(texts):
        n = len(t) - ignore
        if n < 1:      # nothing scored: zeros from the layer, and no line from the tool (shorter than its minimum length)
            assert not mean[k].any() and not stddev[k].any()
            continue
        m_k = sums[k] / n
        sd_k = np.sqrt(np.maximum(0.0, sumsqs[k] / n - m_k * m_k))
        assert np.array_equal(mean[k], m_k) and np.allclose(stddev[k], sd_k, rtol=1e-12, atol=1e-15)
        assert abs(mean[k].sum() - 1.0) < 1e-5 and np.all(stddev[k] > 0)
        want_lines.append("%s mean: %s stddev: %s" % (names[k], "".join("%.3e " % x for x in mean[k]),
                                                       "".join("%.3e " % x for x in stddev[k])))
    tool = os.path.join(rc.ROOT, "build", "text_classify_results_amd")
    r = subprocess.run([tool, "-f", path, "-i", str(ignore)] + names, capture_output=True, text=True, timeout=120,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.splitlines() == want_lines and len(want_lines) == 3
    r = subprocess.run([tool, "-f", path, "-i", str(ignore), "-m", "100"] + names[::-1], capture_output=True, text=True,
                       timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.splitlines() == [want_lines[2], want_lines[0]]   # the order of the files changes no figure
