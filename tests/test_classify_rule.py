"""The per-row rule of rnn_amd_classify_texts and the arithmetic that finishes its sums, asked of the rule itself
(recur_amd/csrc/classify_rule.h) without a GPU: classify_rule_harness.cpp is compiled with g++ alone, lays a batch over
state rows as the call does (texts_plan.h handed every length plus one), walks the waves launch by launch as the call's
host loop does and prints at which steps every text is fed, scored and counted; it prints which class bytes are valid, and
the mean and standard deviation for given sums.  All of it is held to a numpy restatement of the rules; the restatement is
then broken one rule at a time to show that each rule is noticed.  The same program runs under the address and
undefined-behaviour sanitizers (it has its own main; nothing is preloaded).  And the refusals and the no-device early
returns of the call and of its character layer, through the loaded library."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import recur_ctypes as rc

ROOT = rc.ROOT
CSRC = os.path.join(ROOT, "recur_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "classify_rule_harness.cpp")
NO_CLASS = 0xFF
LENS = [0, 1, 2, 3, 7, 7, 12, 1, 0, 5]
SKIPS = [0, 0, 1, 3, 2, 9, 0, 1, 4, -2]     # a skip == len, one > len, a negative one
CLASSES = [0, NO_CLASS, 3, 254, NO_CLASS, 1, 0]   # class byte of (text k, step t): CLASSES[(k + t) % 7]
WIDTHS = [1, 3, 256]
RULES = ["the_last_symbol_is_fed", "a_step_is_scored_from_its_skip_on", "a_skip_beyond_the_text_scores_nothing",
         "only_0xff_is_no_class", "a_class_names_an_output", "n_is_len_minus_ignore_start", "the_mean_divides_by_n",
         "the_variance_is_clamped_at_zero", "nothing_scored_gives_zeros"]
# (len, sum, sumsq) under IGNORE = 2; the second is three symbols of probability 0.1: sumsq / n - mean * mean is below zero
IGNORE = 2
FINISH = [(12, 4.5, 2.5), (5, 0.1 + 0.1 + 0.1, 0.03), (3, 0.25, 0.0625), (2, 0.0, 0.0), (0, 0.0, 0.0), (9, 7.0, 7.0)]


def build(tmp_path_factory, name, extra=()):
    exe = str(tmp_path_factory.mktemp(name) / "classify_rule_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I", CSRC, SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build(tmp_path_factory, "classify_rule")


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return build(tmp_path_factory, "classify_rule_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def run(exe, *args):
    return subprocess.run([exe, *map(str, args)], capture_output=True, text=True, check=True).stdout


def ints(v):
    return [int(x) for x in v.split(",") if x]


def ask_rows(exe, width, lens=LENS, skips=SKIPS, classes=CLASSES):
    out = run(exe, "rows", width, ",".join(map(str, lens)), ",".join(map(str, skips)), ",".join(map(str, classes)))
    return {k: ints(v) for k, v in (line.split("=", 1) for line in out.splitlines())}


def restated_rows(lens=LENS, skips=SKIPS, classes=CLASSES, broken=None):
    d = {}
    for k, (n, skip) in enumerate(zip(lens, skips)):
        fed = list(range(n - 1 if broken == "the_last_symbol_is_fed" else n))
        if broken == "a_step_is_scored_from_its_skip_on":
            scored = [t for t in fed if t > skip]
        elif broken == "a_skip_beyond_the_text_scores_nothing":
            scored = [t for t in fed if t >= min(skip, n - 1)]
        else:
            scored = [t for t in fed if t >= skip]
        none = 0 if broken == "only_0xff_is_no_class" else NO_CLASS
        counted = [t for t in scored if classes[(k + t) % len(classes)] != none]
        d["fed%d" % k], d["scored%d" % k], d["counted%d" % k] = fed, scored, counted
        d["rule%d" % k] = [len(fed), len(scored), len(counted)]
    return d


def restated_class(outputs, broken=None):
    top = outputs + 1 if broken == "a_class_names_an_output" else outputs
    none = 0 if broken == "only_0xff_is_no_class" else NO_CLASS
    return {"ok": sorted(set(range(min(top, 256))) | {NO_CLASS}), "has": [b for b in range(256) if b != none]}


def restated_finish(cases=FINISH, ignore=IGNORE, broken=None):
    out = []
    for n_symbols, s, sq in cases:
        n = max(n_symbols - ignore - (1 if broken == "n_is_len_minus_ignore_start" else 0), 0)
        if n < 1:
            out.append((n, 0.0, 0.0) if broken != "nothing_scored_gives_zeros" else (n, math.nan, math.nan))
            continue
        mean = s / (n + 1 if broken == "the_mean_divides_by_n" else n)
        var = sq / n - mean * mean
        if broken == "the_variance_is_clamped_at_zero":
            out.append((n, mean, math.sqrt(var) if var >= 0 else math.nan))
        else:
            out.append((n, mean, math.sqrt(max(0.0, var))))
    return out


def ask_class(exe, outputs):
    return {k: ints(v) for k, v in (line.split("=", 1) for line in run(exe, "class", outputs).splitlines())}


def ask_finish(exe, cases=FINISH, ignore=IGNORE):
    out = run(exe, "finish", ignore, *["%d:%.17g:%.17g" % c for c in cases])
    return [(int(a), float(b), float(c)) for a, b, c in (line.split() for line in out.splitlines())]


def same_figures(a, b):
    return len(a) == len(b) and all(x[0] == y[0] and all((math.isnan(p) and math.isnan(q)) or p == q for p, q in zip(x[1:], y[1:]))
                                    for x, y in zip(a, b))


def test_the_header_is_plain_c_and_cxx_without_hip():
    for cc, lang in (("gcc", "c"), ("g++", "c++")):
        subprocess.run([cc, "-fsyntax-only", "-Wall", "-Werror", "-Wno-unused-function", "-I", CSRC, "-x", lang,
                        os.path.join(CSRC, "classify_rule.h")], check=True)


def check(exe):
    for width in WIDTHS:   # the width changes rows and waves and no answer (the harness returns 3 where the walk of
        assert ask_rows(exe, width) == restated_rows(), width   # the plan and classify_fed / _scored / _counted differ)
    # every (len, skip, t) of small texts, and skips at and beyond every length
    lens = [n for n in range(0, 7) for _ in range(-1, 9)]
    skips = [s for _ in range(0, 7) for s in range(-1, 9)]
    assert ask_rows(exe, 4, lens, skips, [NO_CLASS, 1]) == restated_rows(lens, skips, [NO_CLASS, 1])
    for outputs in (1, 2, 5, 200, 255, 256, 300):
        assert ask_class(exe, outputs) == restated_class(outputs), outputs
    assert same_figures(ask_finish(exe), restated_finish())


def test_fed_scored_counted_class_bytes_and_the_finish_are_the_restated_ones(harness):
    check(harness)
    got = restated_rows()
    assert got["fed4"] == list(range(7)) and got["scored4"] == list(range(2, 7))   # every symbol fed, the last included
    assert got["scored3"] == [] and got["fed3"] == [0, 1, 2]                       # skip == len: fed, never scored
    assert got["scored5"] == [] and got["scored9"] == got["fed9"]                  # skip > len; a negative skip
    assert got["fed0"] == [] and got["fed1"] == [0]


def test_the_clamp_case_really_lies_below_zero(harness):
    n_symbols, s, sq = FINISH[1]
    n = n_symbols - IGNORE
    assert sq / n - (s / n) * (s / n) < 0.0                  # what the reference's expression would take the root of
    got = ask_finish(harness)[1]
    assert got == (3, s / 3, 0.0)
    assert ask_finish(harness)[3] == (0, 0.0, 0.0) and ask_finish(harness)[4] == (0, 0.0, 0.0)   # nothing scored
    assert ask_finish(harness)[5][2] == math.sqrt(1.0 - 1.0)                                       # certainty: no spread


@pytest.mark.parametrize("broken", RULES)
def test_each_rule_is_noticed(harness, broken):
    differ = ask_rows(harness, 3) != restated_rows(broken=broken)
    differ += any(ask_class(harness, o) != restated_class(o, broken) for o in (5, 200, 256))
    differ += not same_figures(ask_finish(harness), restated_finish(broken=broken))
    assert differ >= 1, broken


def test_under_address_and_undefined_behaviour_sanitizers(sanitized):
    """stand-alone: the harness has its own main, the sanitizers' runtimes are linked into it"""
    check(sanitized)


# ------------------------------------------------------------------ the call's refusals need no device --

@pytest.fixture(scope="module")
def lib():
    return rc.bind_char(rc.load_amd())


def test_refusals_and_early_returns_need_no_device(lib):
    """-1 with nothing written, and 0 where no text has a symbol, on a machine without a GPU (no compute entry point is
    reached; with a device present the same calls return before they touch it)"""
    net = lib.rnn_new(13, 39, 7, rc.FLAG_STANDARD, 1, None, 4, 1e-3, 0.9, 0.0, rc.RELU)
    bottom = lib.rnn_new_with_bottom_layer(20, 13, 39, 7, rc.FLAG_STANDARD, 5, None, 4, 1e-3, 0.9, 0.0, rc.RELU, 0)
    H = net.contents.h_size
    keep = []

    def u8s(*rows):
        arrays = [None if r is None else np.array(r, np.uint8) for r in rows]
        keep.append(arrays)
        return (rc.c_u8_p * len(rows))(*[None if a is None else rc.u8ptr(a) for a in arrays])

    def ints32(*x):
        keep.append(np.array(x, np.int32))
        return rc.iptr(keep[-1])

    h_in = np.random.default_rng(1).random((2, H)).astype(np.float32)
    h_out = np.full((2, H), 5.0, np.float32)
    sums, sumsqs = np.full(2 * 7, 7.0), np.full(2 * 7, 7.0)
    scores = (rc.ClassScore * 2)()
    for s in scores:
        s.error, s.count = 7.0, 7
    dp = C.POINTER(C.c_double)

    def call(net=net, texts=u8s([1, 2, 12], [0, 5]), lens=ints32(3, 2), skips=ints32(0, 1),
             classes=u8s([0, NO_CLASS, 6], [3, 3]), n=2, h_in=rc.fptr(h_in), h_out=rc.fptr(h_out),
             sums=sums.ctypes.data_as(dp), sumsqs=sumsqs.ctypes.data_as(dp), scores=scores):
        return lib.rnn_amd_classify_texts(net, texts, lens, skips, classes, n, h_in, h_out, sums, sumsqs, scores)

    assert call(net=None) == -1 and call(n=-1) == -1
    assert call(net=bottom) == -1                                                   # a bottom layer
    assert call(texts=None) == -1 and call(lens=None) == -1 and call(sums=None) == -1   # NULL arrays for n_texts > 0
    assert call(lens=ints32(3, -1)) == -1                                           # a negative length
    assert call(texts=u8s([1, 2, 12], None)) == -1                                  # a NULL text with symbols
    assert call(texts=u8s([1, 2, 13], [0, 5])) == -1                                # a symbol >= input_size
    assert call(classes=u8s([0, NO_CLASS, 7], [3, 3])) == -1                        # a class byte >= output_size
    assert call(classes=u8s([0, NO_CLASS, 0xFE], None)) == -1
    assert call(skips=ints32(5, 5), classes=u8s(None, [3, 9])) == -1                # ... also where nothing would be scored
    assert np.all(sums == 7.0) and np.all(sumsqs == 7.0) and np.all(h_out == 5.0)
    assert all(s.error == 7.0 and s.count == 7 for s in scores)
    # nothing to run: 0, and no device is asked for
    assert call(n=0, texts=None, lens=None, skips=None, classes=None, h_in=None, h_out=None, sums=None, sumsqs=None,
                scores=None) == 0
    assert np.all(sums == 7.0)                                                      # n_texts == 0 touches nothing
    assert call(lens=ints32(0, 0), texts=u8s(None, None), classes=u8s(None, None)) == 0
    # ... the sums and the scores of texts without a symbol are zeros
    assert np.all(sums == 0.0) and np.all(sumsqs == 0.0)
    assert all((s.error, s.entropy, s.correct, s.count) == (0.0, 0.0, 0, 0) for s in scores)
    # ... and h_out is the start state: elements 1 .. hidden_size of h_in, by the host alone
    assert np.array_equal(h_out[:, 1:40], h_in[:, 1:40])
    same = h_in.copy()
    assert call(lens=ints32(0, 0), h_out=rc.fptr(same), h_in=rc.fptr(same)) == 0    # in place
    assert np.array_equal(same[:, 1:40], h_in[:, 1:40])
    # with h_in NULL it is the net's hidden row, which only the host has here; everything optional left out
    rc.view(net.contents.hidden_layer, H)[1:40] = np.arange(39, dtype=np.float32)
    assert call(lens=ints32(0, 0), h_in=None, skips=None, classes=None, sumsqs=None, scores=None) == 0
    assert np.array_equal(h_out[:, 1:40], np.tile(np.arange(39, dtype=np.float32), (2, 1)))
    for x in (bottom, net):
        lib.rnn_delete_net(x)


def test_the_character_layer_refuses_before_it_needs_a_device(lib):
    net = lib.rnn_new(13, 39, 7, rc.FLAG_STANDARD, 1, None, 4, 1e-3, 0.9, 0.0, rc.RELU)
    bottom = lib.rnn_new_with_bottom_layer(20, 13, 39, 7, rc.FLAG_STANDARD, 5, None, 4, 1e-3, 0.9, 0.0, rc.RELU, 0)
    alphabet = rc.default_text_alphabet(lib)     # 42 symbols: more than the net's 13 inputs
    raw = [b"to be or not to be", b"that is"]
    texts = (C.c_char_p * 2)(*raw)
    nbytes = np.array([len(r) for r in raw], np.int32)
    mean, stddev = np.full(2 * 7, 7.0), np.full(2 * 7, 7.0)
    dp = C.POINTER(C.c_double)

    def call(net=net, alphabet=alphabet, texts=texts, nbytes=rc.iptr(nbytes), n=2, ignore=0, mean=mean.ctypes.data_as(dp),
             stddev=stddev.ctypes.data_as(dp)):
        return lib.rnn_amd_char_classify_texts(net, alphabet, texts, nbytes, n, ignore, mean, stddev)

    assert call(net=None) == -1 and call(n=-1) == -1 and call(alphabet=None) == -1
    assert call(texts=None) == -1 and call(nbytes=None) == -1 and call(mean=None) == -1
    assert call(texts=(C.c_char_p * 2)(raw[0], None)) == -1
    neg = np.array([3, -1], np.int32)
    assert call(nbytes=rc.iptr(neg)) == -1
    assert call(net=bottom) == -1            # rnn_amd_classify_texts's refusals pass through: a bottom layer,
    assert call() == -1                      # ... a symbol the net has no input for
    assert np.all(mean == 7.0) and np.all(stddev == 7.0)
    assert call(n=0, texts=None, nbytes=None, mean=None, stddev=None) == 0
    # texts that encode to no symbol: zeros, by the host alone
    empty = np.array([0, 0], np.int32)
    assert call(nbytes=rc.iptr(empty)) == 0 and np.all(mean == 0.0) and np.all(stddev == 0.0)
    lib.rnn_char_free_alphabet(alphabet)
    for x in (bottom, net):
        lib.rnn_delete_net(x)
