"""How rnn_amd_run_sequences stages the frames of a batch of dense sequences, asked of the rule itself
(recur_amd/csrc/seqs_plan.h) without a GPU: seqs_plan_harness.cpp is compiled with g++ alone, prints the plan -- order,
waves, segments, live rows, frame counts and offsets -- for the frame counts, wave width and segment length on its command
line, and stages every frame through a buffer of exactly the planned size.  The plan is held to a numpy restatement of the
rules; the restatement is then broken one rule at a time to show that each rule is noticed.  The same program runs under the
address and undefined-behaviour sanitizers (it has its own main; nothing is preloaded).  And the refusals and the
no-device early returns of the call, through the loaded library."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import recur_ctypes as rc

ROOT = rc.ROOT
CSRC = os.path.join(ROOT, "recur_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "seqs_plan_harness.cpp")
FRAMES = [0, 1, 2, 7, 8, 9, 600]
ORDERS = [FRAMES, FRAMES[::-1], [8, 600, 0, 9, 1, 7, 2], [7, 7, 0, 600, 7, 8, 9, 2, 1, 600, 0, 8]]
WIDTHS = [1, 3, 256]
SEGMENTS = [1, 4, 8, 601, 5000]   # 601 and 5000: larger than the longest sequence
STAGE_BYTES = 2 << 20             # seqs_plan.h's SEQS_STAGE_BYTES, stated here a second time
RULES = ["order_stable", "no_frame_no_row", "segments_round_up", "live_is_strict", "count_is_clamped_above",
         "count_is_clamped_below", "offsets_exclude_the_row", "largest_is_the_first_segment", "default_fits_the_budget"]


def build(tmp_path_factory, name, extra=()):
    exe = str(tmp_path_factory.mktemp(name) / "seqs_plan_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I", CSRC, SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build(tmp_path_factory, "seqs_plan")


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return build(tmp_path_factory, "seqs_plan_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def ask(exe, width, segment, input_size, frames):
    out = subprocess.run([exe, str(width), str(segment), str(input_size), ",".join(map(str, frames))],
                         capture_output=True, text=True, check=True).stdout
    d = dict(line.split("=", 1) for line in out.splitlines())
    return {k: [int(x) for x in v.split(",")] if v else [] for k, v in d.items()}


def restated(width, segment, input_size, frames, broken=None):
    """seqs_plan.h's rules in numpy, as the dictionary the harness prints; `broken` names the one rule left out"""
    W = width if width >= 1 else 256
    default = max(STAGE_BYTES // (W * max(input_size, 1) * 4), 1)
    if broken == "default_fits_the_budget":
        default += 1
    F = segment if segment > 0 else default
    frames = np.asarray(frames, np.int64)
    takes = frames >= (0 if broken == "no_frame_no_row" else 1)
    idx = np.flatnonzero(takes)
    if broken == "order_stable":
        idx = idx[::-1]
    order = idx[np.argsort(-frames[idx], kind="stable")]
    rows = frames[order]
    d = {"segment": [F], "default": [default], "n_rows": [len(rows)], "n_waves": [-(-len(rows) // W)],
         "order": list(map(int, order)), "frames": list(map(int, rows))}
    hits = [np.zeros(n, int) for n in frames]
    largest = 0
    for w in range(d["n_waves"][0]):
        mine = rows[w * W:(w + 1) * W]
        steps = int(mine[0])
        d["wave%d" % w] = [w * W, len(mine), steps]
        nseg = steps // F if broken == "segments_round_up" else -(-steps // F)
        d["segments%d" % w] = [nseg]
        for q in range(nseg):
            t0 = q * F
            live = int((mine >= t0).sum() if broken == "live_is_strict" else (mine > t0).sum())
            count = mine - t0
            if broken != "count_is_clamped_above":
                count = np.minimum(count, F)
            if broken != "count_is_clamped_below":
                count = np.maximum(count, 0)
            off = np.cumsum(count) if broken == "offsets_exclude_the_row" else np.cumsum(count) - count
            total = int(count.sum())
            d["seg%d_%d" % (w, q)] = [t0, min(F, steps - t0), live, total]
            d["count%d_%d" % (w, q)] = list(map(int, count))
            d["off%d_%d" % (w, q)] = list(map(int, off))
            largest = max(largest, total)
            if w == 0 and q == (1 if broken == "largest_is_the_first_segment" and nseg > 1 else 0):
                d["largest"] = [total]
            for j in range(live):
                hits[order[w * W + j]][t0:t0 + max(int(count[j]), 0)] += 1
    d.setdefault("largest", [0])
    if broken is None:
        assert d["largest"] == [largest]  # the first segment of the first wave IS the largest
    every = np.concatenate(hits) if len(hits) else np.zeros(0, int)
    d["hits"] = [int(every.min()), int(every.max())] if every.size and every.max() > 0 else [0, 0]
    return d


CONFIGS = [(w, f, 32, order) for w, f, order in itertools.product(WIDTHS, SEGMENTS, ORDERS)] + \
          [(256, 0, 32, FRAMES), (256, 0, 13, FRAMES), (3, -1, 1 << 20, FRAMES), (0, 0, 32, FRAMES), (256, 0, 0, [])]


def test_the_header_is_plain_c_and_cxx_without_hip():
    for cc, lang in (("gcc", "c"), ("g++", "c++")):
        subprocess.run([cc, "-fsyntax-only", "-Wall", "-Werror", "-Wno-unused-function", "-I", CSRC, "-x", lang,
                        os.path.join(CSRC, "seqs_plan.h")], check=True)


def check(exe, configs=CONFIGS):
    for width, segment, input_size, frames in configs:
        got = ask(exe, width, segment, input_size, frames)
        assert got == restated(width, segment, input_size, frames), (width, segment, input_size, frames)
        # every (row, frame) lands in exactly one segment slot: the harness staged them, and from the printed tables
        if sum(frames):
            assert got["hits"] == [1, 1]
        seen = {}
        for w in range(got["n_waves"][0]):
            row0, nrows, steps = got["wave%d" % w]
            for q in range(got["segments%d" % w][0]):
                t0, length, live, total = got["seg%d_%d" % (w, q)]
                count, off = got["count%d_%d" % (w, q)], got["off%d_%d" % (w, q)]
                assert 1 <= length <= got["segment"][0] and 1 <= live <= nrows and total <= got["largest"][0]
                assert all(c >= 1 for c in count[:live]) and not any(count[live:])    # the live rows are a prefix
                slots = [o + i for o, c in zip(off, count) for i in range(c)]
                assert slots == list(range(total))                                    # dense, no slot twice
                for j in range(live):
                    for i in range(count[j]):
                        key = (got["order"][row0 + j], t0 + i)
                        assert key not in seen
                        seen[key] = (w, q, off[j] + i)
        assert sorted(seen) == [(k, t) for k, n in enumerate(frames) for t in range(n)]


def test_segments_live_rows_and_offsets_are_the_restated_ones(harness):
    check(harness)


def test_the_default_segment_keeps_a_waves_input_staging_within_the_budget(harness):
    for width, input_size in [(256, 32), (256, 13), (256, 1), (3, 32), (256, 1 << 20)]:
        got = ask(harness, width, 0, input_size, FRAMES)
        f = got["default"][0]
        assert got["segment"] == [f] and f >= 1
        assert f == 1 or width * f * input_size * 4 <= STAGE_BYTES < width * (f + 1) * input_size * 4
    assert ask(harness, 256, 0, 32, FRAMES)["default"] == [64]
    assert ask(harness, 256, 7, 32, FRAMES)["segment"] == [7]


def test_the_buffers_go_by_the_largest_segment_not_the_longest_sequence(harness):
    got = ask(harness, 256, 8, 32, FRAMES)
    assert got["largest"] == [1 + 2 + 7 + 8 + 8 + 8] and got["segments0"] == [75]
    assert ask(harness, 256, 601, 32, FRAMES)["largest"] == [sum(FRAMES)]
    assert ask(harness, 1, 8, 32, FRAMES)["largest"] == [8]


@pytest.mark.parametrize("broken", RULES)
def test_each_rule_is_noticed(harness, broken):
    differ = 0
    for width, segment, input_size, frames in CONFIGS:
        try:
            differ += ask(harness, width, segment, input_size, frames) != restated(width, segment, input_size, frames, broken)
        except (ValueError, IndexError):
            differ += 1   # the broken restatement does not even hold together
    assert differ >= 1, broken


def test_under_address_and_undefined_behaviour_sanitizers(sanitized):
    """stand-alone: the harness has its own main, the sanitizers' runtimes are linked into it.  Its staging buffer has
    exactly the planned size, so a slot outside it is an error here"""
    check(sanitized)


# ------------------------------------------------------------------ the call's refusals need no device --

@pytest.fixture(scope="module")
def lib():
    return rc.bind_char(rc.load_amd())


def test_refusals_and_early_returns_need_no_device(lib):
    """-1 with nothing written, and 0 where no sequence has a frame, on a machine without a GPU (no compute entry point is
    reached; with a device present the same calls return before they touch it)"""
    net = lib.rnn_new(13, 39, 7, rc.FLAG_STANDARD, 1, None, 4, 1e-3, 0.9, 0.0, rc.RELU)
    bottom = lib.rnn_new_with_bottom_layer(20, 13, 39, 7, rc.FLAG_STANDARD, 5, None, 4, 1e-3, 0.9, 0.0, rc.RELU, 0)
    H = net.contents.h_size
    feats = [np.ones((3, 13), np.float32), np.ones((2, 13), np.float32)]
    inp = (rc.c_float_p * 2)(*[rc.fptr(a) for a in feats])
    frames = np.array([3, 2], np.int32)
    ans = [np.full(3 * 7, 7.0, np.float32), np.full(2 * 7, 7.0, np.float32)]
    win = [np.full(3 * 2, 0xEE, np.uint8), np.full(2 * 2, 0xEE, np.uint8)]
    ansp = (rc.c_float_p * 2)(*[rc.fptr(a) for a in ans])
    winp = (rc.c_u8_p * 2)(*[rc.u8ptr(a) for a in win])
    goff, gsize = np.array([0, 3], np.int32), np.array([2, 4], np.int32)
    h_in = np.random.default_rng(1).random((2, H)).astype(np.float32)
    h_out = np.full((2, H), 5.0, np.float32)

    def call(net=net, inputs=inp, frames=rc.iptr(frames), n=2, ld=13, ng=2, goff=rc.iptr(goff), gsize=rc.iptr(gsize),
             h_in=rc.fptr(h_in), h_out=rc.fptr(h_out), segment=0, answers=ansp, winners=winp):
        return lib.rnn_amd_run_sequences(net, inputs, frames, n, ld, ng, goff, gsize, h_in, h_out, segment, answers, winners)

    def ints(*x):
        a = np.array(x, np.int32)
        call.keep = getattr(call, "keep", []) + [a]
        return rc.iptr(a)

    assert call(net=None) == -1
    assert call(n=-1) == -1 and call(ng=-1) == -1 and call(frames=ints(3, -1)) == -1     # negative counts
    assert call(net=bottom) == -1                                                          # a bottom layer
    assert call(goff=ints(0, 1)) == -1                                                     # groups that overlap
    assert call(goff=ints(0, 4)) == -1 and call(goff=ints(-1, 3)) == -1                    # ... that leave the row
    assert call(gsize=ints(2, 0)) == -1                                                    # ... without a class
    assert call(gsize=ints(2, 5)) == -1
    assert call(ld=12) == -1                                                               # rows too narrow
    assert call(inputs=None) == -1 and call(frames=None) == -1 and call(answers=None) == -1
    assert call(goff=None) == -1 and call(gsize=None) == -1
    assert call(inputs=(rc.c_float_p * 2)(rc.fptr(feats[0]), None)) == -1                  # a NULL row of an array
    assert call(answers=(rc.c_float_p * 2)(None, rc.fptr(ans[1]))) == -1
    assert call(winners=(rc.c_u8_p * 2)(rc.u8ptr(win[0]), None)) == -1
    assert call(ng=0, goff=None, gsize=None) == -1                                         # winners without a group
    wide = lib.rnn_new(13, 39, 300, rc.FLAG_STANDARD, 1, None, 4, 1e-3, 0.9, 0.0, rc.RELU)
    big = [np.full(3 * 300, 7.0, np.float32), np.full(2 * 300, 7.0, np.float32)]
    bigp = (rc.c_float_p * 2)(*[rc.fptr(a) for a in big])
    assert call(net=wide, ng=1, goff=ints(0), gsize=ints(257), answers=bigp, h_in=None, h_out=None) == -1   # 257 classes
    assert all(np.all(a == 7.0) for a in ans + big) and all(np.all(a == 0xEE) for a in win) and np.all(h_out == 5.0)
    # nothing to run: 0, and no device is asked for
    assert call(n=0, inputs=None, frames=None, answers=None, winners=None, h_in=None, h_out=None) == 0
    assert call(frames=ints(0, 0), inputs=(rc.c_float_p * 2)(None, None), answers=(rc.c_float_p * 2)(None, None),
                winners=(rc.c_u8_p * 2)(None, None)) == 0
    # ... and h_out is the start state: elements 1 .. hidden_size of h_in, by the host alone
    assert np.array_equal(h_out[:, 1:40], h_in[:, 1:40])
    same = h_in.copy()
    assert call(frames=ints(0, 0), h_out=rc.fptr(same), h_in=rc.fptr(same)) == 0           # in place
    assert np.array_equal(same[:, 1:40], h_in[:, 1:40])
    # with h_in NULL it is the net's hidden row, which only the host has here
    rc.view(net.contents.hidden_layer, H)[1:40] = np.arange(39, dtype=np.float32)
    assert call(frames=ints(0, 0), h_in=None) == 0
    assert np.array_equal(h_out[:, 1:40], np.tile(np.arange(39, dtype=np.float32), (2, 1)))
    assert all(np.all(a == 7.0) for a in ans) and all(np.all(a == 0xEE) for a in win)
    for x in (wide, bottom, net):
        lib.rnn_delete_net(x)
