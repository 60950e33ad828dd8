"""rnnca's automaton played on the device (rnn_amd_run_automaton; recur_amd/csrc/automaton_api.c, automaton_rule.h,
k_automaton_step in kernels_rows.hip) against the oracle: an OracleSet with one stream per cell, the product's weights
copied in (both get the same seeded numpy weights), every stream starting from the product net's hidden row or from its
h_in row, then per frame fill_frame's loop body (gstrnnca.c:805-831): the cell's inputs gathered by a numpy restatement
of fill_net_inputs (the vectorised twin of test_automaton_rule.input_rows, held to it below), orc_opinion with noise 0,
orc_fast_sigmoid on three outputs.

THE COMPARISON is teacher-forced, as test_gpu_sample_texts': for frame t the oracle's cells are fed the inputs gathered
from the DEVICE's frame t - 1 (the seed for t = 0); their hidden rows are their own.  A frame is bytes, so a pixel is
judged by how far the parity bar lets its scaled value move: with the oracle's output o, a = sigmoid(o), v = a * 255.9f
and R the largest |output| of that frame's oracle outputs, the margin is m = 255.9 a (1 - a) 1e-4 R + 1e-4 -- the bar's
1e-4 of the largest output through the sigmoid's slope, and 1e-4 of a level for the float32 roundings of the product.  A
pixel is CLEAR when floor(v - m) == floor(v + m): the device's byte must be floor(v).  Otherwise it must be one of the
two.  No pixel may differ from floor(v) by more than one level.  Levels are bytes: a floor below 0 is level 0 (a is never
negative, so v - m < 0 names no other level; without this every pixel of the saturated case with v = 5e-20 would count as
unclear), one above 255 is level 255.  h_out is held to the oracle's hidden rows at the project's parity bar
(test_gpu_trace_texts.at_the_bar).

UNCLEAR PIXELS are at most 2 % of each case's pixels, a condition on the nets: for evenly spread fractional parts the
share is about 2 m <= 0.0128 R, so outputs with R <= 1.5 stay under the cap, and the cases' top layers are scaled to that.
The unmarked tests assert it from the oracle alone, free-running from the same seed, and that each case's last oracle
frame still holds at least 16 distinct luma levels (on the 3 x 3 grid, which has nine pixels, nine) and that consecutive
frames differ: a net that has settled on one colour tests nothing.  The device tests assert the cap again on the teacher-forced run.

Where two calls must agree they agree bit for bit: the same call twice, the segment length, NULL against explicit start
states, a cut joined through the last frame and h_out -> h_in in place.

The oracle's runs are computed once per case and shared."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import recur_ctypes as rc
import scenarios as sc
from recur_amd.drivers import AutomatonGeometry, run_automaton
from test_automaton_rule import DEFAULT_C, DEFAULT_Y, input_rows
from test_fwd_plan import CXX as PLAN_CXX, SRC as PLAN_SRC, plan
from test_gpu_trace_texts import at_the_bar

gpu = pytest.mark.gpu
F = np.float32
CAP = 0.02
GAIN = 2.0
POS_GAIN = 12.0
_cases = {}
_free = {}
_forced = {}
_nets = {}


class Case:
    """a grid, a net (seeded numpy weights, a seeded hidden row, half of it zeros as a rectifier leaves it) and a seed
    frame of random bytes.  saturated: the top layer is written, not learned -- hidden unit 1 keeps what the cell's start
    state gives it (0 or 1) and switches the three outputs between (-50, 50, -1e4) and (50, -50, 1e4)"""

    def __init__(self, name, width, height, hidden, frames, seed, edges=1, len_pos=2, top=1.0, segment=0, saturated=False):
        self.name, self.width, self.height, self.hidden, self.frames = name, width, height, hidden, frames
        self.edges, self.len_pos, self.segment, self.saturated = edges, len_pos, segment, saturated
        self.cells = width * height
        self.inputs = len(DEFAULT_Y) + 2 * len(DEFAULT_C) + len_pos
        g = np.random.default_rng(seed)
        sizes = [C.c_int(0) for _ in range(3)]
        rc.load_oracle().orc_padded_sizes(self.inputs, hidden, 3, *[C.byref(x) for x in sizes])
        self.I, self.H, self.O = [x.value for x in sizes]
        self.ih = np.zeros((self.I, self.H), np.float32)
        self.ho = np.zeros((self.H, self.O), np.float32)
        self.h_in = None
        if saturated:
            self.ih[2, 2] = 1.0                       # hidden unit 1 (column 2 of the row [bias, h0, h1, ...]) keeps itself
            self.ho[0, :3] = [-50.0, 50.0, -1e4]      # (row 0 of W_ho is the bias)
            self.ho[2, :3] = [100.0, -100.0, 2e4]
            self.row = np.zeros(self.H, np.float32)
            self.row[0] = 1.0
            self.h_in = np.tile(self.row, (self.cells, 1))
            self.h_in[::3, 2] = 1.0
            self.h_in[7, 2] = 1.0
        else:
            # bias row 0.1, recurrent rows 1 / sqrt(hidden), input rows GAIN / sqrt(inputs) (bytes are units in [0, 1]) and
            # the position's rows POS_GAIN times that: a neighbourhood of +-2 on a grid of 5 x 4 is nearly the whole frame,
            # so without a strong sense of place the cells soon paint one colour.  W_ho is top / sqrt(hidden): `top`
            # brings the largest output under 1.5.  Seeds and `top` were chosen on the free-running oracle, which the
            # unmarked tests below repeat
            self.ih[0, 1:1 + hidden] = 0.1 * g.standard_normal(hidden)
            self.ih[1:1 + hidden, 1:1 + hidden] = g.standard_normal((hidden, hidden)) / np.sqrt(hidden)
            self.ih[1 + hidden:1 + hidden + self.inputs, 1:1 + hidden] = g.standard_normal((self.inputs, hidden)) * (GAIN / np.sqrt(self.inputs))
            self.ih[1 + hidden + self.inputs - len_pos:1 + hidden + self.inputs, 1:1 + hidden] *= POS_GAIN
            self.ho[:1 + hidden, :3] = g.standard_normal((1 + hidden, 3)) * (top / np.sqrt(hidden))
            self.row = self.state(g)
        self.seed = g.integers(0, 256, (3, height, width), dtype=np.uint8)
        self.geometry = AutomatonGeometry(width, height, DEFAULT_Y, DEFAULT_C, len_pos, edges)
        assert self.geometry.input_size == self.inputs
        self.index_y = self.sources(DEFAULT_Y)
        self.index_c = self.sources(DEFAULT_C)

    def state(self, g):
        h = np.zeros(self.H, np.float32)
        h[0] = 1.0
        h[1:1 + self.hidden] = np.maximum(g.standard_normal(self.hidden), 0.0) * 0.5
        return h

    def sources(self, offsets):
        """gstrnnca.c:644-667 for every offset and cell at once: [offsets][cells]"""
        w, h = self.width, self.height
        cy, cx = np.divmod(np.arange(self.cells), w)
        out = []
        for dx, dy in offsets:
            x, y = cx + dx, cy + dy
            if self.edges:
                x, y = np.clip(x, 0, w - 1), np.clip(y, 0, h - 1)
            else:
                x = np.where(x < 0, x + w, np.where(x >= w, x - w, x))
                y = np.where(y < 0, y + h, np.where(y >= h, y - h, y))
            out.append(y * w + x)
        return np.array(out)

    def gather(self, frame):
        """gstrnnca.c:669-691 for every cell at once: the input rows [cells][inputs] float32 from a frame [3][h][w]"""
        planes = frame.reshape(3, self.cells)
        recip = F(1.0) / F(255.0)
        ly, lc = len(DEFAULT_Y), len(DEFAULT_C)
        rows = np.empty((self.cells, self.inputs), F)
        rows[:, :ly] = planes[0][self.index_y].T.astype(F) * recip
        rows[:, ly:ly + 2 * lc:2] = planes[1][self.index_c].T.astype(F) * recip
        rows[:, ly + 1:ly + 2 * lc:2] = planes[2][self.index_c].T.astype(F) * recip
        cy, cx = np.divmod(np.arange(self.cells), self.width)
        xx = cx.astype(F) * F(1.0) / F(self.width)
        yy = cy.astype(F) * F(1.0) / F(self.height)
        rows[:, ly + 2 * lc] = xx
        rows[:, ly + 2 * lc + 1] = yy
        if self.len_pos == 3:
            x64, y64 = xx.astype(np.float64), yy.astype(np.float64)
            rows[:, ly + 2 * lc + 2] = (0.5 - ((y64 - 0.5) * (y64 - 0.5) + (x64 - 0.5) * (x64 - 0.5))).astype(F)
        return rows


def case(name):
    if name not in _cases:
        made = {
            # 5 x 4 cells under offsets to +-2: every cell touches an edge
            "small_clamp": lambda: Case(name, 5, 4, 32, 6, 38, top=0.2),
            "small_wrap": lambda: Case(name, 5, 4, 32, 6, 38, edges=0, top=0.2),
            "tiny_wrap": lambda: Case(name, 3, 3, 32, 6, 37, edges=0, top=0.15),
            "pos3": lambda: Case(name, 5, 4, 32, 6, 23, len_pos=3, top=0.2),
            # more rows than any scratch-row call has run, an odd hidden size
            "over_wave": lambda: Case(name, 24, 16, 99, 4, 25, top=0.15),
            # 2048 rows at I = 548: nine K stages of 64 -- k_fwd_wide fed from built rows, the 4-column output layer
            "wide": lambda: Case(name, 64, 32, 512, 2, 26, top=0.15),
            "full_grid": lambda: Case(name, 144, 96, 64, 2, 27, top=0.1, segment=1),
            "saturated": lambda: Case(name, 5, 4, 32, 3, 28, saturated=True),
        }
        _cases[name] = made[name]()
    return _cases[name]


ALL = ["small_clamp", "small_wrap", "tiny_wrap", "pos3", "over_wave", "wide", "full_grid", "saturated"]


class Judged:
    """one oracle frame: the outputs [cells][3], and per pixel [3][cells] the level floor(v), the two levels the margin
    allows, and whether they are one"""

    def __init__(self, orc, out):
        self.out = out.copy()
        a = np.array([orc.orc_fast_sigmoid(float(x)) for x in out.ravel()], F).reshape(out.shape).T
        v = (a * F(255.9)).astype(np.float64)
        self.R = float(np.abs(out).max())
        a64 = a.astype(np.float64)
        m = 255.9 * a64 * (1.0 - a64) * 1e-4 * self.R + 1e-4

        def level(x):   # levels are bytes
            return np.clip(np.floor(x), 0, 255).astype(np.int64)

        self.level, self.low, self.high = level(v), level(v - m), level(v + m)
        self.clear = self.low == self.high


def oracle_run(c, forced=None, h_in=None, frames=None, seed=None):
    """the oracle's run of a case: free-running from the seed (forced None: frame t is gathered from the oracle's own frame
    t - 1, the bytes being floor(v)) or teacher-forced (forced: the device's frames [n][3][h][w]).  Returns (the list of
    Judged frames, the oracle's frames as bytes, the final hidden rows [cells][H])"""
    n = c.frames if frames is None else frames
    o = sc.OracleSet(input_size=c.inputs, hidden_size=c.hidden, output_size=3, S=c.cells, D=1, learn_rate=1e-3, seed=1)
    assert (o.I, o.H, o.O) == (c.I, c.H, c.O)
    arr = o.arrays()
    arr["ih_w"][:] = c.ih
    arr["ho_w"][:] = c.ho
    start = h_in if h_in is not None else c.h_in
    arr["hidden"][:] = start if start is not None else c.row[None, :]
    judged, painted = [], np.zeros((n, 3, c.height, c.width), np.uint8)
    before = c.seed if seed is None else seed
    for t in range(n):
        rows = c.gather(before)
        for k in range(c.cells):
            o.orc.orc_opinion(o.z, k, rc.fptr(rows[k]), 0.0)
        j = Judged(o.orc, arr["output"][:, :3])
        judged.append(j)
        painted[t] = j.level.astype(np.uint8).reshape(3, c.height, c.width)
        before = painted[t] if forced is None else forced[t]
    hidden = arr["hidden"].copy()
    o.close()
    return judged, painted, hidden


OWN_STATES = ("small_wrap", "pos3")   # the cases that also run with a start state per cell
OWN_SEED = 34


def own_states(c):
    g = np.random.default_rng(OWN_SEED)
    return np.stack([c.state(g) for _ in range(c.cells)])


def free(name):
    if name not in _free:
        _free[name] = oracle_run(case(name))
    return _free[name]


# ------------------------------------------------------------------ the oracle alone: no device --

@pytest.mark.parametrize("name", ALL)
def test_the_chosen_nets_keep_the_unclear_pixels_under_the_cap_and_stay_alive(name):
    c = case(name)
    judged, painted, _ = free(name)
    unclear = sum(int((~j.clear).sum()) for j in judged)
    pixels = 3 * c.cells * c.frames
    R = max(j.R for j in judged)
    luma = len(np.unique(painted[-1][0]))
    print("%s: %d pixels, %d unclear (%.3f %%), largest |output| %.3g, %d luma levels in the last frame"
          % (name, pixels, unclear, 100.0 * unclear / pixels, R, luma))
    assert unclear <= CAP * pixels
    if c.saturated:   # outputs of +-50 and +-1e4: bytes 0 and 255, and nothing else
        assert R == 1e4 and sorted(np.unique(painted)) == [0, 255]
        assert sorted(np.unique(np.abs(np.concatenate([j.out.ravel() for j in judged])))) == [50.0, 1e4]
        assert len(np.unique(painted[-1][0])) == 2 and len(np.unique(painted[-1][1])) == 2
        return
    assert R <= 1.5
    assert luma >= min(16, c.cells)   # (the 3 x 3 grid has nine pixels: every one its own level)
    assert not np.array_equal(painted[0], c.seed)
    assert all(not np.array_equal(painted[t], painted[t + 1]) for t in range(c.frames - 1))


@pytest.mark.parametrize("name", OWN_STATES)
def test_the_cap_holds_with_a_start_state_per_cell_too(name):
    c = case(name)
    judged, painted, _ = oracle_run(c, h_in=own_states(c))
    unclear = sum(int((~j.clear).sum()) for j in judged)
    print("%s, a start state per cell: %d pixels, %d unclear, largest |output| %.3g" % (name, 3 * c.cells * c.frames, unclear, max(j.R for j in judged)))
    assert unclear <= 0.5 * CAP * 3 * c.cells * c.frames   # (half the cap: the teacher-forced run is another trajectory)
    assert max(j.R for j in judged) <= 1.5 and not np.array_equal(painted, free(name)[1])


def test_the_vectorised_gather_is_the_restatement_the_rule_is_held_to():
    for name in ("small_clamp", "small_wrap", "tiny_wrap", "pos3"):
        c = case(name)
        want = input_rows(c.seed.ravel(), c.width, c.height, c.edges, c.len_pos, DEFAULT_Y, DEFAULT_C)
        assert np.array_equal(c.gather(c.seed).view(np.uint32), want.view(np.uint32)), name


def test_the_wide_case_gets_the_wide_kernel_from_built_rows_and_the_four_column_output_layer(tmp_path):
    """asked of fwd_plan.h itself: 2048 forward-only rows whose input rows k_automaton_step has built, I = 548 (nine K
    stages of 64), O = 4; the workspace as the engine sizes it (16 planes of every state row's sums, engine.c)"""
    c = case("wide")
    exe = str(tmp_path / "fwd_plan_harness")
    subprocess.run(PLAN_CXX + [PLAN_SRC, "-o", exe], check=True)
    p = plan(exe, input=c.inputs, hidden=c.hidden, output=3, streams=1, fwd_only=0, row0=1, nrows=c.cells, mode=0, advance=0,
             rows_built=1, slab_floats=16 * (1 + c.cells) * c.H)
    assert (p["I"], p["H"], p["O"]) == (c.I, c.H, c.O) == (548, 516, 4)
    assert (p["input"], p["hidden"], p["ns"], p["tm"], p["tn"], p["end"], p["output"]) == ("built", "wide", 9, 32, 9, "finalize", "o4")
    # a row fewer than 2048, or a net a stage narrower, would not reach it
    assert plan(exe, input=c.inputs, hidden=c.hidden, output=3, streams=1, row0=1, nrows=c.cells - 64, mode=0, advance=0,
                rows_built=1)["hidden"] == "gemm"
    assert plan(exe, input=c.inputs, hidden=440, output=3, streams=1, row0=1, nrows=c.cells, mode=0, advance=0,
                rows_built=1)["hidden"] == "gemm"


# ------------------------------------------------------------------ the device --

@pytest.fixture(scope="module")
def amd():
    lib = rc.bind_char(rc.load_amd())
    assert lib.rnn_amd_device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return lib


def product(lib, name):
    """the case's net in the product: made once and shared, never changed after this"""
    if name not in _nets:
        c = case(name)
        net = lib.rnn_new(c.inputs, c.hidden, 3, rc.FLAG_STANDARD, 1, None, 4, 1e-3, 0.9, 0.0, rc.RELU)
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


def run(lib, name, n_frames=None, seed=None, **kw):
    """run_automaton on the case's net and grid (with its own start states and segment), the net unchanged by the call"""
    c, net = case(name), product(lib, name)
    before = snapshot(lib, net)
    if c.h_in is not None:
        kw.setdefault("h_in", c.h_in)
    kw.setdefault("segment_frames", c.segment)
    got = run_automaton(lib, net, c.geometry, c.seed if seed is None else seed, c.frames if n_frames is None else n_frames, **kw)
    after = snapshot(lib, net)
    assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(before, after)), name
    return got


def held_to_the_oracle(c, frames, judged, what):
    """every pixel of the device's frames against the teacher-forced oracle frames; returns (unclear, pixels)"""
    unclear = differ = 0
    for t, j in enumerate(judged):
        mine = frames[t].reshape(3, c.cells).astype(np.int64)
        assert np.all(np.abs(mine - j.level) <= 1), (what, t, np.argwhere(np.abs(mine - j.level) > 1)[:5])
        assert np.array_equal(mine[j.clear], j.level[j.clear]), (what, t, np.argwhere((mine != j.level) & j.clear)[:5])
        assert np.all((mine == j.low) | (mine == j.high)), (what, t)
        unclear += int((~j.clear).sum())
        differ += int((mine != j.level).sum())
    pixels = 3 * c.cells * len(judged)
    print("%s: %d pixels, %d unclear (%.3f %%), %d not the oracle's level, largest |output| %.3g"
          % (what, pixels, unclear, 100.0 * unclear / max(pixels, 1), differ, max(j.R for j in judged)))
    assert unclear <= CAP * pixels
    return unclear, pixels


def states_at_the_bar(c, h_out, hidden, what):
    assert h_out.shape == (c.cells, c.H)
    for k in range(c.cells):
        at_the_bar(np.ascontiguousarray(h_out[k, 1:1 + c.hidden]), np.ascontiguousarray(hidden[k, 1:1 + c.hidden]),
                   "%s, state of cell %d" % (what, k))


def forced(lib, name):
    """(the device's frames and states of the case, the oracle teacher-forced with those frames), once per case"""
    if name not in _forced:
        frames, h_out = run(lib, name)
        _forced[name] = (frames, h_out, oracle_run(case(name), forced=frames))
    return _forced[name]


def same_bits(a, b, c):
    (fa, ha), (fb, hb) = a, b
    return np.array_equal(fa, fb) and np.array_equal(ha[:, 1:1 + c.hidden].view(np.uint32), hb[:, 1:1 + c.hidden].view(np.uint32))


# ------------------------------------------------------------------ 1. every case against the oracle --

@gpu
@pytest.mark.parametrize("name", ALL)
def test_frames_and_states_meet_the_oracle(amd, name):
    c = case(name)
    frames, h_out, (judged, _, hidden) = forced(amd, name)
    assert frames.shape == (c.frames, 3, c.height, c.width) and frames.dtype == np.uint8
    held_to_the_oracle(c, frames, judged, name)
    states_at_the_bar(c, h_out, hidden, name)
    if c.saturated:
        assert sorted(np.unique(frames)) == [0, 255] and (frames[-1][0].ravel() == 255).sum() == 8
    else:
        assert len(np.unique(frames[-1][0])) >= min(16, c.cells) and not np.array_equal(frames[0], frames[-1])


# ------------------------------------------------------------------ 2. bit for bit --

@gpu
def test_the_same_call_twice_writes_every_byte_and_the_same_bytes(amd):
    """the frame arrays of the two calls start as different bytes: a byte that was not written would differ"""
    for name in ("small_clamp", "over_wave"):
        c = case(name)
        first = run(amd, name, fill=0xEE)    # (the driver asserts the guards behind the frames and behind the states)
        again = run(amd, name, fill=0x11)
        assert same_bits(first, again, c), name
        assert same_bits(first, forced(amd, name)[:2], c), name


@gpu
def test_the_segment_size_changes_no_bit(amd):
    c = case("small_wrap")
    whole = run(amd, "small_wrap")                       # the default: one segment here
    for segment in (1, 3, 4, 6, 1000):                   # 6 frames as 6 x 1, 3 + 3, 4 + 2, one
        assert same_bits(run(amd, "small_wrap", segment_frames=segment), whole, c), segment
    assert same_bits(whole, forced(amd, "small_wrap")[:2], c)
    full = case("full_grid")                             # whose own segment is 1
    assert same_bits(run(amd, "full_grid", segment_frames=0), forced(amd, "full_grid")[:2], full)


@gpu
def test_null_states_are_the_nets_hidden_row(amd):
    for name in ("small_clamp", "over_wave"):
        c = case(name)
        filled = run(amd, name, h_in=np.tile(c.row, (c.cells, 1)))
        assert same_bits(filled, forced(amd, name)[:2], c), name


@gpu
def test_a_run_cut_in_two_and_joined_in_place_is_the_uncut_run(amd):
    """6 frames against 2 + 4, joined by the last frame as the next seed and by the states, updated where they lie"""
    for name in OWN_STATES:
        c = case(name)
        start = own_states(c)
        uncut, h_uncut = run(amd, name, h_in=start)
        state = start.copy()
        first, h1 = run(amd, name, n_frames=2, h_in=state, in_place=True)
        assert h1 is not None and np.shares_memory(h1, state) and not np.array_equal(state, start)
        second, h2 = run(amd, name, n_frames=4, seed=first[-1], h_in=state, in_place=True)
        assert np.array_equal(np.concatenate([first, second]), uncut), name
        assert np.array_equal(state[:, 1:1 + c.hidden].view(np.uint32), h_uncut[:, 1:1 + c.hidden].view(np.uint32)), name
        # and distinct start states meet the oracle as the shared one does
        judged, _, hidden = oracle_run(c, forced=uncut, h_in=start)
        held_to_the_oracle(c, uncut, judged, name + ", a start state per cell")
        states_at_the_bar(c, h_uncut, hidden, name + ", a start state per cell")
    # no frames: the states come back as they went in, and no frame is written (the driver's guards begin at byte 0)
    none, h_none = run(amd, "small_wrap", n_frames=0, h_in=start)
    assert none.shape == (0, 3, 4, 5) and np.array_equal(h_none[:, 1:33], start[:, 1:33])


# ------------------------------------------------------------------ 3. the net is left alone --

@gpu
def test_the_net_computes_next_what_a_twin_that_made_no_call_computes(amd):
    """(run() asserts for every call that hidden row, generator and weights are unchanged on both sides)"""
    lib, c = amd, case("small_clamp")
    twins = []
    for _ in range(2):
        net = lib.rnn_new(c.inputs, c.hidden, 3, rc.FLAG_STANDARD, 1, None, 4, 1e-3, 0.9, 0.0, rc.RELU)
        n = net.contents
        rc.view(n.ih_weights, c.I, c.H)[:] = c.ih
        rc.view(n.ho_weights, c.H, c.O)[:] = c.ho
        lib.rnn_amd_host_written(net, rc.RNN_AMD_WEIGHTS)
        lib.rnn_amd_sync_host(net, rc.RNN_AMD_STREAM)
        rc.view(n.hidden_layer, c.H)[:] = c.row
        lib.rnn_amd_host_written(net, rc.RNN_AMD_STREAM)
        twins.append(net)
    caller, idle = twins
    frames, _ = run_automaton(lib, caller, c.geometry, c.seed, c.frames)
    assert np.array_equal(frames, forced(lib, "small_clamp")[0])
    x = c.gather(c.seed)[7]
    answers = []
    for net in (caller, idle):
        out = lib.rnn_opinion(net, rc.fptr(x), 0.0)
        answers.append(rc.view(out, c.O)[:3].copy())
        lib.rnn_amd_sync_host(net, rc.RNN_AMD_STREAM)
        answers.append(rc.view(net.contents.hidden_layer, c.H)[1:1 + c.hidden].copy())
    assert np.array_equal(answers[0].view(np.uint32), answers[2].view(np.uint32))
    assert np.array_equal(answers[1].view(np.uint32), answers[3].view(np.uint32))
    assert np.any(answers[0] != 0.0)
    for net in twins:
        lib.rnn_delete_net(net)


# ------------------------------------------------------------------ 4. against today's loop --

@gpu
def test_one_frame_against_todays_per_frame_loop(amd):
    """the recipe the call replaces: gather on the host, rnn_amd_set_opinion over one forward-only clone per cell,
    rnn_amd_set_sigmoid_outputs, the host's byte conversion -- from the same seed and the same states.  Bytes are equal on
    every pixel the oracle calls clear and within one level elsewhere (the two paths run the forward pass in different
    kernel forms)"""
    lib, name = amd, "small_clamp"
    c, net = case(name), product(amd, name)
    frames, _, (judged, _, _) = forced(lib, name)
    fl = net.contents.flags & ~(rc.FLAG_OWN_WEIGHTS | rc.FLAG_OWN_BPTT)
    cells = (rc.NetP * c.cells)()
    for k in range(c.cells):
        cells[k] = lib.rnn_clone(net, fl, rc.SUBSEED, None)
        lib.rnn_amd_sync_host(cells[k], rc.RNN_AMD_STREAM)
        rc.view(cells[k].contents.hidden_layer, c.H)[:] = c.row
        lib.rnn_amd_host_written(cells[k], rc.RNN_AMD_STREAM)
    handle = lib.rnn_amd_set_open(cells, c.cells)
    assert handle
    out = np.zeros((c.cells, c.O), np.float32)
    rows = np.ascontiguousarray(c.gather(c.seed))
    lib.rnn_amd_set_opinion(handle, rc.fptr(rows), c.inputs, None)
    lib.rnn_amd_set_sigmoid_outputs(handle, 3, rc.fptr(out))
    scaled = out[:, :3] * F(255.9)
    loop = np.clip(np.floor(scaled), 0, 255).astype(np.int64).T    # [3][cells]
    mine = frames[0].reshape(3, c.cells).astype(np.int64)
    j = judged[0]
    assert np.array_equal(loop[j.clear], mine[j.clear]) and np.all(np.abs(loop - mine) <= 1)
    assert np.array_equal(loop[j.clear], j.level[j.clear])
    print("today's loop: %d of %d pixels differ from the call's, %d unclear" % ((loop != mine).sum(), loop.size, (~j.clear).sum()))
    lib.rnn_amd_set_close(handle)
    for k in range(c.cells):
        lib.rnn_delete_net(cells[k])


# ------------------------------------------------------------------ 5. the tool --

def jenkins_bytes(seed, count):
    """count bytes from a generator seeded init_rand64(seed) (recur-rng.h:22-43), the words as they lie in memory"""
    M = (1 << 64) - 1

    def rot(x, k):
        return ((x << k) | (x >> (64 - k))) & M

    a, b, c, d = 0xF1EA5EED, seed, seed, seed
    words = []
    for i in range(20 + (count + 7) // 8):
        e = (a - rot(b, 7)) & M
        a = b ^ rot(c, 13)
        b = (c + rot(d, 37)) & M
        c = (d + e) & M
        d = (e + a) & M
        if i >= 20:
            words.append(d)
    return np.frombuffer(np.array(words, "<u8").tobytes(), np.uint8)[:count].copy()


@gpu
def test_the_tool_writes_the_drivers_bytes(amd, tmp_path):
    lib = amd
    path = str(tmp_path / "rnnca.net")
    assert lib.rnn_save_net(product(lib, "small_clamp"), path.encode(), 0) == 0 and os.path.exists(path)
    tool = os.path.join(rc.ROOT, "build", "rnnca_play_amd")
    seed_file = str(tmp_path / "seed.u8")
    case("small_wrap").seed.tofile(seed_file)
    runs = [(["-w", "5", "-h", "4", "-n", "3", "-s", "7"], case("small_clamp").geometry, jenkins_bytes(7, 60)),
            (["-w", "5", "-h", "4", "-n", "2", "-E", "-i", seed_file], case("small_wrap").geometry, case("small_wrap").seed)]
    for args, geometry, seed in runs:
        n = int(args[5])
        loaded = lib.rnn_load_net(path.encode())   # the tool starts from the state the file holds: so does the driver
        want, _ = run_automaton(lib, loaded, geometry, seed, n, want_out=False)
        lib.rnn_delete_net(loaded)
        out = str(tmp_path / "frames.yuv")
        r = subprocess.run([tool] + args + [path, out], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-2000:]
        got = np.fromfile(out, np.uint8)
        assert got.size == n * 60 and np.array_equal(got, want.ravel()), args
        assert len(np.unique(got)) > 16
    r = subprocess.run([tool, "-w", "2", "-h", "4", "-E", path, str(tmp_path / "none.yuv")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 1 and "single wrap" in r.stderr and not os.path.exists(str(tmp_path / "none.yuv"))
