"""Many dense feature sequences against one net in one batched device run (rnn_amd_run_sequences;
recur_amd/csrc/seqs_api.c, seqs_plan.h, k_seqs_step in kernels_rows.hip) against the oracle: an OracleSet with one stream
per sequence, the product's weights copied in (both get the same seeded numpy weights), every stream starting from the
product net's hidden row or from its h_in row, then per frame orc_opinion with noise 0 and per class group orc_softmax and
orc_softmax_best_guess -- emit_opinions' loop body (gstclassify.c:2273-2280).  A sequence's expected answers are what
orc_softmax_best_guess stores, negated back, inside a group and orc_opinion's output in every other column.

THE BAR is the project's parity bar, applied per sequence to its answers array (test_gpu_trace_texts.at_the_bar: 1e-4 on
the 2-norm and on the largest element, element by element 1e-4 relative on the elements of at least 1e-2 of the array's
largest, the bound of an element at that floor below it).  THE WINNERS are teacher-checked
(test_gpu_trace_texts.teacher_checked): the oracle's likelihood at the device's pick lies within 1e-4, relative, of the
oracle's largest; where the oracle's best leads its runner-up by more than that the pick is the oracle's; and at most 1 %
of a test's picks may lie where the lead is 1e-4 or less.  That the chosen inputs keep to that cap, and that the soft-clip
case really exceeds I * INPUT_MEAN_SOFT_TOP, is asserted from the oracle alone, without a device (the two unmarked tests).

Where two calls must agree they agree bit for bit: the segment length, NULL against explicit start states, a cut joined by
h_out -> h_in in place, the caller's order.  The same row counts per pass launch the same kernels on the same rows.

The oracle's results are computed once per case and shared."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import recur_ctypes as rc
import scenarios as sc
from recur_amd.drivers import run_sequences
from test_gpu_trace_texts import BAR, at_the_bar, margins, teacher_checked

gpu = pytest.mark.gpu
SOFT_TOP = 16.0   # INPUT_MEAN_SOFT_TOP (recur-nn.h)
BASE_GROUPS = [(0, 2), (3, 4)]   # the class string "01,abcd": column 2 is the comma, in no group
_cases = {}
_wants = {}
_nets = {}


class Case:
    """a net (seeded numpy weights, a seeded hidden row, half of it zeros as a rectifier leaves it) and a batch of
    sequences; own_states: every sequence starts from a state of its own (h_in) instead of the net's hidden row"""

    def __init__(self, name, inputs, hidden, outputs, groups, frames, seed, activation=rc.RELU, amp=1.0, top=1.0,
                 loud=(), own_states=False):
        self.name, self.inputs, self.hidden, self.outputs, self.groups = name, inputs, hidden, outputs, list(groups)
        self.frames, self.seed, self.activation, self.own_states = list(frames), seed, activation, own_states
        g = np.random.default_rng(seed)
        sizes = [C.c_int(0) for _ in range(3)]
        rc.load_oracle().orc_padded_sizes(inputs, hidden, outputs, *[C.byref(x) for x in sizes])
        self.I, self.H, self.O = [x.value for x in sizes]
        # test_gpu_texts_wide.seeded_net's weights with dense inputs: bias row 0.1, recurrent rows 1 / sqrt(hidden), input
        # rows 1 / sqrt(inputs) (hidden values of about 1 from features of about 1), W_ho top / sqrt(hidden)
        self.ih = np.zeros((self.I, self.H), np.float32)
        self.ho = np.zeros((self.H, self.O), np.float32)
        self.ih[0, 1:1 + hidden] = 0.1 * g.standard_normal(hidden)
        self.ih[1:1 + hidden, 1:1 + hidden] = g.standard_normal((hidden, hidden)) / np.sqrt(hidden)
        self.ih[1 + hidden:1 + hidden + inputs, 1:1 + hidden] = g.standard_normal((inputs, hidden)) / np.sqrt(inputs)
        self.ho[:1 + hidden, :outputs] = g.standard_normal((1 + hidden, outputs)) * (top / np.sqrt(hidden))
        self.row = self.state(g)
        self.h_in = np.stack([self.state(g) for _ in frames]) if own_states else None
        self.seqs = [(amp * g.standard_normal((n, inputs))).astype(np.float32) for n in self.frames]
        for k in loud:  # every feature far on the positive side: the input row's sum passes the soft clip
            self.seqs[k] = (150.0 + 10.0 * g.standard_normal((self.frames[k], inputs))).astype(np.float32)
        self.loud = set(loud)

    def state(self, g):
        h = np.zeros(self.H, np.float32)
        h[0] = 1.0
        h[1:1 + self.hidden] = np.maximum(g.standard_normal(self.hidden), 0.0) * 0.5
        return h


# frame counts that make the passes of one call run at 256, 192, 128, 64, 63 and 1 rows (test_gpu_texts_wide.LENS, a
# frame less than a text's symbols), and 4 sequences more: a second wave
WIDE_FRAMES = [1] * 64 + [2] * 64 + [3] * 64 + [4] + [5] * 62 + [6] + [1] * 4
WIDE_ROWS = [256, 192, 128, 64, 63, 1]


def case(name):
    if name not in _cases:
        six = [(4 * i, 3) for i in range(6)]
        wide_frames = [int(x) for x in np.random.default_rng(3).permutation(WIDE_FRAMES)]
        made = {
            "base": lambda: Case(name, 13, 99, 7, BASE_GROUPS, [40, 0, 1, 2, 33, 40, 7, 0], 11),
            "one70": lambda: Case(name, 13, 99, 70, [(0, 70)], [5, 3, 1, 0], 12),            # wider than a wave
            "six3": lambda: Case(name, 13, 99, 23, six, [5, 3, 1], 13),                      # more groups than waves
            "64_65": lambda: Case(name, 13, 99, 130, [(0, 64), (65, 65)], [5, 3, 1], 14),    # a wave exactly, and one more
            "clip": lambda: Case(name, 13, 99, 7, BASE_GROUPS, [6, 9, 4], 15, top=0.05, loud=[1]),
            "states": lambda: Case(name, 13, 99, 7, BASE_GROUPS, [20, 13, 20, 7, 1, 0, 16], 16, own_states=True),
            "wide": lambda: Case(name, 32, 1024, 2, [(0, 2)], wide_frames, 17),
            "resqrt": lambda: Case(name, 13, 99, 7, BASE_GROUPS, [12, 5, 0, 9], 18, activation=rc.RESQRT),
            "reclip20": lambda: Case(name, 13, 99, 7, BASE_GROUPS, [12, 5, 0, 9], 19, activation=rc.RECLIP20, amp=30.0,
                                     top=0.1),
        }
        _cases[name] = made[name]()
    return _cases[name]


class Want:
    """the oracle's run of a case: per sequence raw [n][outputs], answers [n][outputs], best [n][groups], like (a list
    per group of [n][size]), sums [n] (each frame's input-row sum before the clip), and h_out [n_seqs][H]"""


def want(name):
    if name not in _wants:
        c = case(name)
        n = len(c.seqs)
        o = sc.OracleSet(input_size=c.inputs, hidden_size=c.hidden, output_size=c.outputs, S=n, D=1,
                         activation=c.activation, learn_rate=1e-3, seed=1)
        assert (o.I, o.H, o.O) == (c.I, c.H, c.O)
        arr = o.arrays()
        arr["ih_w"][:] = c.ih
        arr["ho_w"][:] = c.ho
        arr["hidden"][:] = c.h_in if c.own_states else c.row[None, :]
        w = Want()
        w.raw, w.answers, w.best, w.like, w.sums = [], [], [], [], []
        for k, seq in enumerate(c.seqs):
            raw = np.zeros((len(seq), c.outputs), np.float32)
            best = np.zeros((len(seq), len(c.groups)), np.int64)
            like = [np.zeros((len(seq), size), np.float32) for _, size in c.groups]
            sums = np.zeros(len(seq))
            for t, frame in enumerate(seq):
                sums[t] = 1.0 + float(arr["hidden"][k, 1:1 + c.hidden].astype(np.float64).sum()) + float(frame.astype(np.float64).sum())
                out = o.orc.orc_opinion(o.z, k, rc.fptr(np.ascontiguousarray(frame)), 0.0)
                raw[t] = np.ctypeslib.as_array(out, shape=(o.O,))[:c.outputs]
            answers = raw.copy()
            for g, (off, size) in enumerate(c.groups):
                err = np.zeros(size, np.float32)
                for t in range(len(seq)):
                    src = np.ascontiguousarray(raw[t, off:off + size])
                    o.orc.orc_softmax(rc.fptr(like[g][t]), rc.fptr(src), size)
                    best[t, g] = o.orc.orc_softmax_best_guess(rc.fptr(err), rc.fptr(src), size)
                    answers[t, off:off + size] = -err   # what softmax_best_guess stores, negated back
            w.raw.append(raw), w.answers.append(answers), w.best.append(best), w.like.append(like), w.sums.append(sums)
        w.h_out = arr["hidden"].copy()
        o.close()
        _wants[name] = w
    return _wants[name]


def unclear(name):
    """(picks where the oracle's best leads its runner-up by 1e-4 of itself or less, picks) of a case"""
    c, w = case(name), want(name)
    close = picks = 0
    for like in w.like:
        for g in range(len(c.groups)):
            if like[g].size:
                close += int((margins(like[g])[1] <= BAR).sum())
                picks += len(like[g])
    return close, picks


ALL = ["base", "one70", "six3", "64_65", "clip", "states", "wide", "resqrt", "reclip20"]


# ------------------------------------------------------------------ the oracle alone: no device --

@pytest.mark.parametrize("name", ALL)
def test_the_chosen_inputs_keep_the_unclear_winners_under_the_cap(name):
    close, picks = unclear(name)
    c, w = case(name), want(name)
    print("%s: %d picks, %d with the oracle's best within 1e-4 of the runner-up" % (name, picks, close))
    assert picks == sum(c.frames) * len(c.groups) and close <= 0.01 * picks
    # and the answers are a classifier's: every group's probabilities add up to one, not every pick is the same class
    for ans, best in zip(w.answers, w.best):
        for off, size in c.groups:
            assert np.allclose(ans[:, off:off + size].sum(axis=1), 1.0, atol=1e-5)
    if picks >= 20:
        assert len(np.unique(np.concatenate([b[:, 0] for b in w.best]))) >= 2
    if name == "reclip20":   # the activation's ceiling is met
        assert np.any(w.h_out[:, 1:1 + c.hidden] == 20.0)
    if name == "wide":       # the design: one call's passes at 256, 192, 128, 64, 63 and 1 rows, and a second wave
        first = sorted(c.frames, reverse=True)[:256]
        assert [sum(n > t for n in first) for t in range(max(first))] == WIDE_ROWS and len(c.frames) == 260


def test_the_soft_clip_case_really_exceeds_the_clip():
    c, w = case("clip"), want("clip")
    top = c.I * SOFT_TOP
    print("clip at %g; input-row sums: %s" % (top, [(round(s.min()), round(s.max())) for s in w.sums]))
    assert all(np.all(w.sums[k] > top) == (k in c.loud) for k in range(len(c.seqs)))
    assert all(np.all(w.sums[k] < 0.5 * top) for k in range(len(c.seqs)) if k not in c.loud)
    for name in ("base", "states", "resqrt", "reclip20"):   # the other hidden-99 cases stay under it
        assert all(np.all(s < case(name).I * SOFT_TOP) for s in want(name).sums)


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


def run(lib, name, seqs=None, **kw):
    """run_sequences on the case's net with its groups (and its own start states), the net unchanged by the call"""
    c, net = case(name), product(lib, name)
    before = snapshot(lib, net)
    kw.setdefault("groups", c.groups)
    if c.own_states:
        kw.setdefault("h_in", c.h_in)
    got = run_sequences(lib, net, c.seqs if seqs is None else seqs, **kw)
    after = snapshot(lib, net)
    assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(before, after)), name
    return got


def held_to_the_oracle(name, got, h_out, w=None, what=None):
    """answers at the bar, winners teacher-checked and under the cap, h_out at the bar"""
    c, w, what = case(name), w or want(name), what or name
    assert [a.shape for a, _ in got] == [(n, c.outputs) for n in c.frames]
    worst = np.zeros(3)
    for k, (ans, _) in enumerate(got):
        worst = np.maximum(worst, at_the_bar(ans, w.answers[k], "%s, sequence %d" % (what, k)))
    print("%s: %d sequences, %d frames, largest differences: 2-norm %.3g, largest element %.3g, element by element %.3g"
          % (what, len(got), sum(c.frames), *worst))
    close = steps = 0
    for g, (_, size) in enumerate(c.groups):
        mine = [(None, win[:, g:g + 1]) for _, win in got]
        theirs = [(None, w.best[k][:, g:g + 1], w.like[k][g][:, None, :]) for k in range(len(got))]
        a, b = teacher_checked(mine, theirs, "%s, group %d of %d classes" % (what, g, size))
        close, steps = close + a, steps + b
    assert steps == sum(c.frames) * len(c.groups) and close <= 0.01 * steps
    if h_out is not None:
        assert h_out.shape == (len(c.seqs), c.H) and not np.any(np.isnan(h_out[:, 1:1 + c.hidden]))
        for k in range(len(c.seqs)):
            at_the_bar(h_out[k, 1:1 + c.hidden], w.h_out[k, 1:1 + c.hidden], "%s, state %d" % (what, k))


def same_bits(a, b):
    (ga, ha), (gb, hb) = a, b
    assert len(ga) == len(gb)
    for (x, wx), (y, wy) in zip(ga, gb):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)) and np.array_equal(wx, wy)
    return True


def states_equal(c, ha, hb):
    return np.array_equal(ha[:, 1:1 + c.hidden].view(np.uint32), hb[:, 1:1 + c.hidden].view(np.uint32))


# ------------------------------------------------------------------ 1. the base case --

@gpu
def test_the_base_case(amd):
    """hidden 99 and 13 inputs (I needs padding), 7 outputs as groups of 2 and 4 around one gap column, sequences of
    40, 0, 1, 2, 33, 40, 7 and 0 frames"""
    c, w = case("base"), want("base")
    got, h_out = run(amd, "base")   # (the driver asserts the guards behind every array and that every entry was written)
    held_to_the_oracle("base", got, h_out)
    for k, (ans, win) in enumerate(got):
        assert win.shape == (c.frames[k], 2) and win.dtype == np.uint8
        at_the_bar(np.ascontiguousarray(ans[:, 2]), np.ascontiguousarray(w.raw[k][:, 2]), "the gap column, sequence %d" % k)
        assert np.all(win[:, 0] < 2) and np.all(win[:, 1] < 4)
    # the sequences without a frame get their start state back: the net's hidden row
    for k in (1, 7):
        assert np.array_equal(h_out[k, 1:1 + c.hidden], c.row[1:1 + c.hidden])
    # no groups: every column is rnn_opinion's answer; the gap column is the same float in both calls
    raw, h_raw = run(amd, "base", groups=None)
    for k, (ans, win) in enumerate(raw):
        assert win is None
        at_the_bar(ans, w.raw[k], "raw outputs, sequence %d" % k)
        assert np.array_equal(ans[:, 2], got[k][0][:, 2])
    assert states_equal(c, h_raw, h_out)
    # without winners the answers are the same bits, and h_out may be left out
    quiet, none = run(amd, "base", winners=False, want_out=False)
    assert none is None and all(win is None and np.array_equal(a, b) for (a, win), (b, _) in zip(quiet, got))


# ------------------------------------------------------------------ 2. the limits of group width and group count --

@gpu
@pytest.mark.parametrize("name", ["one70", "six3", "64_65"])
def test_group_width_and_group_count(amd, name):
    """one group of 70 classes, wider than a wave; six groups of 3, more groups than the kernel has waves, with gap
    columns between them; groups of 64 and 65 classes"""
    got, h_out = run(amd, name)
    held_to_the_oracle(name, got, h_out)
    c, w = case(name), want(name)
    covered = np.zeros(c.outputs, bool)
    for off, size in c.groups:
        covered[off:off + size] = True
    for k, (ans, _) in enumerate(got):
        if (~covered).any() and len(ans):
            at_the_bar(np.ascontiguousarray(ans[:, ~covered]), np.ascontiguousarray(w.raw[k][:, ~covered]), "gap columns")


# ------------------------------------------------------------------ 3. segmentation is invisible --

@gpu
def test_segmentation_is_invisible(amd):
    """segments of 1, 4 and 8 frames against the unsegmented call, bit for bit: 40 and 8 frames are multiples of the
    segment, 33 and 9 exceed one by 1"""
    c = case("base")
    g = np.random.default_rng(5)
    seqs = c.seqs + [g.standard_normal((n, 13)).astype(np.float32) for n in (8, 9, 16, 4, 5)]
    whole = run(amd, "base", seqs, segment_frames=1000)
    assert same_bits(whole, run(amd, "base", seqs))   # the default: one segment here too
    for segment in (1, 4, 8):
        cut = run(amd, "base", seqs, segment_frames=segment)
        assert same_bits(cut, whole) and states_equal(c, cut[1], whole[1]), segment
    held_to_the_oracle("base", whole[0][:8], whole[1][:8])   # (the sequences do not see one another)


# ------------------------------------------------------------------ 4. states --

@gpu
def test_null_states_are_the_nets_hidden_row(amd):
    c = case("base")
    plain = run(amd, "base")
    filled = run(amd, "base", h_in=np.tile(c.row, (len(c.seqs), 1)))
    assert same_bits(plain, filled) and states_equal(c, plain[1], filled[1])


@gpu
def test_a_cut_joined_through_the_states_in_place_is_the_uncut_call(amd):
    """sequences of equal length cut at one place: both calls' passes run at the same row counts as the uncut call's"""
    c = case("states")
    g = np.random.default_rng(6)
    seqs = [g.standard_normal((24, 13)).astype(np.float32) for _ in range(5)]
    start = np.stack([c.state(g) for _ in seqs])
    (uncut, h_uncut) = run(amd, "states", seqs, h_in=start)
    state = start.copy()
    first, h1 = run(amd, "states", [s[:10] for s in seqs], h_in=state, in_place=True)
    assert h1 is not None and np.shares_memory(h1, state) and not states_equal(c, state, start)
    second, h2 = run(amd, "states", [s[10:] for s in seqs], h_in=state, in_place=True)
    for k in range(len(seqs)):
        assert np.array_equal(np.concatenate([first[k][0], second[k][0]]), uncut[k][0])
        assert np.array_equal(np.concatenate([first[k][1], second[k][1]]), uncut[k][1])
    assert states_equal(c, state, h_uncut)


@gpu
def test_distinct_start_states_and_ragged_chunks_meet_the_oracle(amd):
    c = case("states")
    got, h_out = run(amd, "states")
    held_to_the_oracle("states", got, h_out)
    assert np.array_equal(h_out[5, 1:1 + c.hidden], c.h_in[5, 1:1 + c.hidden])   # no frame: the start state
    # every sequence cut at a place of its own, the second call from the first one's states
    cuts = [7, 13, 0, 3, 1, 0, 15]
    first, h1 = run(amd, "states", [s[:n] for s, n in zip(c.seqs, cuts)])
    second, h2 = run(amd, "states", [s[n:] for s, n in zip(c.seqs, cuts)], h_in=h1)
    joined = [(np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])) for a, b in zip(first, second)]
    held_to_the_oracle("states", joined, h2, what="states, ragged chunks")


# ------------------------------------------------------------------ 5. the order does not matter --

@gpu
def test_a_permuted_batch_gives_the_permuted_results(amd):
    c = case("base")
    got, h_out = run(amd, "base")
    perm = [3, 5, 0, 7, 4, 2, 6, 1]
    again, h_again = run(amd, "base", [c.seqs[k] for k in perm])
    assert same_bits(([got[k] for k in perm], None), (again, None))
    assert states_equal(c, h_again, h_out[perm])


# ------------------------------------------------------------------ 6. the soft clip --

@gpu
def test_a_sequence_over_the_soft_clip_beside_ones_under_it(amd):
    got, h_out = run(amd, "clip")
    held_to_the_oracle("clip", got, h_out)


# ------------------------------------------------------------------ 7. width --

@gpu
def test_hidden_1024_at_every_row_count_and_a_second_wave(amd):
    """hidden 1024, 32 inputs, 2 classes; 260 sequences whose frame counts run one call's passes at 256, 192, 128, 64, 63
    and 1 rows, and a second wave of 4"""
    got, h_out = run(amd, "wide")
    held_to_the_oracle("wide", got, h_out)


@gpu
@pytest.mark.parametrize("name", ["resqrt", "reclip20"])
def test_the_other_activations(amd, name):
    got, h_out = run(amd, name)
    held_to_the_oracle(name, got, h_out)


# ------------------------------------------------------------------ 8. the tool --

@gpu
def test_the_tool_prints_what_the_driver_returns(amd, tmp_path):
    lib, c = amd, case("base")
    net = product(lib, "base")
    m = rc.ClassifyMetadata(b"01,abcd", 100.0, 1600.0, 700.0, 0, 256, b"classify", 0, 600.0, 0.0, 0, 0.0, None, None)
    p = lib.rnn_amd_classify_construct_metadata(C.byref(m))
    keep = C.create_string_buffer(C.string_at(p))
    C.CDLL(None).free(C.c_void_p(p))
    path = str(tmp_path / "classify.net")
    net.contents.metadata = C.cast(keep, C.c_char_p)
    saved = lib.rnn_save_net(net, path.encode(), 0)
    net.contents.metadata = None
    assert saved == 0 and os.path.exists(path)
    seqs = [c.seqs[4][:12], c.seqs[0][:7]]
    names = []
    for k, s in enumerate(seqs):
        names.append(str(tmp_path / ("features%d.f32" % k)))
        s.tofile(names[-1])
    loaded = lib.rnn_load_net(path.encode())   # the tool starts from the state the file holds: so does the driver
    got, _ = run_sequences(lib, loaded, seqs, groups=BASE_GROUPS)
    lib.rnn_delete_net(loaded)
    want_lines = []
    for name, (ans, win) in zip(names, got):
        for t in range(len(ans)):
            words = [name, str(t)]
            for g, (off, size) in enumerate(BASE_GROUPS):
                words.append("01,abcd"[off + int(win[t, g])])
                words += ["%.6f" % float(x) for x in ans[t, off:off + size]]
            want_lines.append(" ".join(words))
    tool = os.path.join(rc.ROOT, "build", "classify_run_amd")
    for args in ([], ["-s", "5"]):
        r = subprocess.run([tool] + args + [path] + names, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.splitlines() == want_lines, args
    assert len(want_lines) == 19
