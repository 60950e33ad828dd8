"""How a text's next symbol is drawn, asked of the rule itself (recur_amd/csrc/sample_rule.h, what k_texts_continue runs
on the device) without a GPU: sample_rule_harness.cpp is compiled with g++ alone, takes the oracle's exponential and generator
(liboracle.so) as the rule's functors and prints the picks and the generator for a row of scores, a bias and a seed.  The
expected values are tests/sample_oracle.py's restatement on the oracle -- orc_softmax twice, a float32 cumulative sum,
orc_rand_double -- and must be met bit for bit: picks, the generator's four words, the number of rand64 steps.  And the
refusals of rnn_amd_sample_texts, which come before anything needs a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import recur_ctypes as rc
import sample_oracle as so

ROOT = rc.ROOT
CSRC = os.path.join(ROOT, "recur_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "sample_rule_harness.cpp")
ORACLE_DIR = os.path.join(ROOT, "oracle")
CXX = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
LINK = ["-L", ORACLE_DIR, "-l:liboracle.so", "-Wl,-rpath," + ORACLE_DIR]
DRAWS = 200


@pytest.fixture(scope="module")
def orc():
    return rc.load_oracle()  # (builds oracle/liboracle.so where it is missing)


def build(tmp_path_factory, name, extra=()):
    exe = str(tmp_path_factory.mktemp(name) / "sample_rule_harness")
    subprocess.run(CXX + list(extra) + [SRC, "-o", exe] + LINK, check=True)
    return exe


@pytest.fixture(scope="module")
def harness(orc, tmp_path_factory):
    return build(tmp_path_factory, "sample_rule")


@pytest.fixture(scope="module")
def sanitized(orc, tmp_path_factory):
    """the same program under AddressSanitizer and UndefinedBehaviorSanitizer: it has its own main, so the runtimes are
    linked into it and nothing is preloaded"""
    return build(tmp_path_factory, "sample_rule_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def ask(exe, score, bias, seed, count):
    args = [exe, repr(float(bias)), str(seed), str(count)] + [float(x).hex() if np.isfinite(x) else "nan" for x in score]
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    d = dict(line.split("=", 1) for line in r.stdout.splitlines())
    return [int(x) for x in d["picks"].split(",")], tuple(int(x) for x in d["rng"].split(",")), int(d["draws"])


def rows(n, rng):
    """rows of n scores: ordinary ones, one with a value above 50, one with a value below -60, one with both, one with
    tied maxima, one whose spread leaves the -60 clamp no room"""
    plain = (3.0 * rng.standard_normal(n)).astype(np.float32)
    high, low, both, tied, wide = plain.copy(), plain.copy(), plain.copy(), plain.copy(), plain.copy()
    high[n // 3] = 71.5
    high[n // 2] = 69.25
    low[n // 4] = -83.0
    both[1] = 55.0
    both[n - 2] = -70.0
    tied[[2, n // 2, n - 1]] = plain.max() + np.float32(0.5)
    wide[0], wide[n - 1] = 48.0, -90.0
    return {"plain": plain, "above 50": high, "below -60": low, "both": both, "tied maxima": tied, "wide": wide}


def want_of(orc, score, bias, seed, count):
    g = so.seeded(orc, seed)
    if bias >= so.GREEDY_BIAS:
        return [so.greedy(score)] * count, so.words(g), 0
    c = so.cumulative(orc, score, bias)
    picks, draws = [], 0
    for _ in range(count):
        pick, us = so.draw(orc, g, c)
        picks.append(pick)
        draws += len(us)
    return picks, so.words(g), draws


def check_parity(exe, orc, count):
    rng = np.random.default_rng(3)
    for n in (14, 42, 73):
        for name, score in rows(n, rng).items():
            for bias in (0.0, 1.0, 200.0):
                seed = 1000 * n + int(bias)
                got = ask(exe, score, bias, seed, count)
                want = want_of(orc, score, bias, seed, count)
                assert got == want, (n, name, bias)
                if bias < so.GREEDY_BIAS:
                    assert got[2] >= count and got[1] != so.words(so.seeded(orc, seed))
                else:
                    assert got[1] == so.words(so.seeded(orc, seed))  # no draw at all
    tied = rows(42, rng)["tied maxima"]
    assert ask(exe, tied, 200.0, 1, 1)[0] == [41]  # the LAST of the three equal maxima


def test_the_header_needs_no_hip():
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-x", "c++",
                    os.path.join(CSRC, "sample_rule.h")], check=True)


def test_picks_and_generator_are_the_oracles_bit_for_bit(harness, orc):
    check_parity(harness, orc, DRAWS)


def test_the_draws_spread_over_the_row(harness, orc):
    """(the parity above is not between two constant answers)"""
    score = np.random.default_rng(3).standard_normal(42).astype(np.float32)  # no symbol rarer than e^-6 or so of the row
    picks, _, _ = ask(harness, score, 0.0, 9, 400)
    assert len(set(picks)) > 20
    sharp, _, _ = ask(harness, score, 1.0, 9, 400)
    assert sharp != picks


def nan_row():
    score = rows(42, np.random.default_rng(4))["plain"]
    score[17] = np.nan
    return score


def check_the_cap(exe, orc):
    for bias in (0.0, 1.0):
        picks, words, draws = ask(exe, nan_row(), bias, 77, 1)
        g = so.seeded(orc, 77)
        for _ in range(so.MAX_ATTEMPTS):
            orc.orc_rand64(C.byref(g))
        assert picks == [-1] and draws == so.MAX_ATTEMPTS == 64 and words == so.words(g)
    # an infinite score never enters the exponential (whose range reduction would not end on it): the same failure
    inf = rows(14, np.random.default_rng(4))["plain"]
    args = [exe, "0.0", "5", "1"] + [float(x).hex() for x in inf[:-1]] + ["inf"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "picks=-1\n" in r.stdout and "draws=64" in r.stdout, r.stderr[-2000:]


def test_a_row_with_a_nan_fails_after_exactly_64_draws(harness, orc):
    check_the_cap(harness, orc)


def test_under_address_and_undefined_behaviour_sanitizers(sanitized, orc):
    """stand-alone: the harness has its own main, the sanitizers' runtimes are linked into it"""
    check_parity(sanitized, orc, 20)
    check_the_cap(sanitized, orc)


def test_refusals_need_no_device():
    """-1 with nothing written, 0 for nothing to draw, on a machine without a GPU (no compute entry point is reached: with
    a device present the same calls return before they touch it)"""
    lib = rc.bind_char(rc.load_amd())
    net = lib.rnn_new(42, 39, 42, rc.FLAG_STANDARD, 1, None, 4, 1e-3, 0.9, 0.0, rc.RELU)
    bottom = lib.rnn_new_with_bottom_layer(42, 16, 39, 42, rc.FLAG_STANDARD, 5, None, 4, 1e-3, 0.9, 0.0, rc.RELU, 0)
    first = np.array([3, 4], np.int32)
    seeds = np.array([1, 2], np.uint64)
    out = np.full((2, 10), 0xEE, np.uint8)
    lens = np.full(2, -7, np.int32)
    sp = seeds.ctypes.data_as(C.POINTER(C.c_uint64))

    def call(net=net, first=rc.iptr(first), seeds=sp, n=2, max_len=10, alen=0, head=0, out=rc.u8ptr(out), lens=rc.iptr(lens)):
        return lib.rnn_amd_sample_texts(net, first, seeds, n, max_len, 0.0, -1, alen, head, out, lens, None)

    assert call(net=bottom) == -1
    assert call(n=-1) == -1 and call(max_len=-1) == -1
    assert call(first=None) == -1 and call(seeds=None) == -1 and call(out=None) == -1 and call(lens=None) == -1
    for bad in (-1, 42, 1000):
        assert call(first=rc.iptr(np.array([3, bad], np.int32))) == -1
    assert call(alen=5) == -1 and call(alen=-14) == -1      # 42 outputs are not heads of 5
    assert call(alen=14, head=3) == -1 and call(alen=14, head=-1) == -1 and call(head=1) == -1
    assert np.all(out == 0xEE) and np.all(lens == -7)       # nothing written
    # nothing to draw: lengths zeroed, no device asked for
    assert call(n=0, first=None, seeds=None, out=None, lens=None) == 0
    assert call(max_len=0) == 0 and list(lens) == [0, 0] and np.all(out == 0xEE)
    # the character layer: refusals pass through, and too little room writes nothing
    alphabet = rc.default_text_alphabet(lib)
    bufs = [C.create_string_buffer(b"\x55" * 8, 8) for _ in range(2)]
    dest = (C.c_char_p * 2)(*[C.cast(b, C.c_char_p) for b in bufs])
    nbytes = np.full(2, -7, np.int32)
    assert lib.rnn_amd_char_confabulate_texts(bottom, alphabet, sp, 2, 5, 0.0, 3, -1, dest, 8, rc.iptr(nbytes)) == -1
    assert lib.rnn_amd_char_confabulate_texts(net, alphabet, sp, -1, 5, 0.0, 3, -1, dest, 8, rc.iptr(nbytes)) == -1
    assert lib.rnn_amd_char_confabulate_texts(net, alphabet, sp, 2, 5, 0.0, 3, -1, dest, 1, rc.iptr(nbytes)) == 0
    assert list(nbytes) == [0, 0] and all(b.raw[0] == 0 and b.raw[1:] == b"\x55" * 7 for b in bufs)
    lib.rnn_char_free_alphabet(alphabet)
    lib.rnn_delete_net(bottom)
    lib.rnn_delete_net(net)


def test_nothing_to_draw_hands_back_the_seeded_generators(orc):
    """max_len == 0 with rng_out: lengths zeroed, no symbol written, generator k init_rand64(seeds[k]), no device asked for"""
    lib = rc.bind_char(rc.load_amd())
    net = lib.rnn_new(42, 39, 42, rc.FLAG_STANDARD, 1, None, 4, 1e-3, 0.9, 0.0, rc.RELU)
    first = np.array([3, 4, 41], np.int32)
    seeds = np.array([1, 2 ** 40 + 5, 0], np.uint64)
    out = np.full((3, 4), 0xEE, np.uint8)
    lens = np.full(3, -7, np.int32)
    rng = np.full((3, 4), 0x5555, np.uint64)
    r = lib.rnn_amd_sample_texts(net, rc.iptr(first), seeds.ctypes.data_as(C.POINTER(C.c_uint64)), 3, 0, 0.0, -1, 0, 0,
                                 rc.u8ptr(out), rc.iptr(lens), rng.ctypes.data_as(C.POINTER(rc.RandCtx)))
    assert r == 0 and list(lens) == [0, 0, 0] and np.all(out == 0xEE)
    assert [tuple(int(x) for x in row) for row in rng] == [so.words(so.seeded(orc, int(s))) for s in seeds]
    lib.rnn_delete_net(net)
