"""How parrot's player turns an answer into the next input, asked of the rule itself (recur_amd/csrc/dream_rule.h, what
k_dream_step runs on the device) without a GPU: dream_rule_harness.cpp is compiled with g++ alone, takes the oracle's
cheap_gaussian_noise (liboracle.so) as the draw's functor and prints or writes what the rule makes of its inputs.  The
expected values are a numpy float32 restatement of badmaths.h:55-68 and gstparrot.c:576 (dream_cases.py) and must be met
bit for bit.  The restatement is then broken one rule at a time, and each broken form must differ on the same inputs: they
would notice that rule being wrong.  Where the reference tree is present, dream_tanh is also held to the reference's own
fast_tanhf, compiled into a temporary directory.  And the refusals and early returns of rnn_amd_dream_sequences, which come
before anything needs a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import recur_ctypes as rc
from dream_cases import (CSRC, EXTREME, F, build_harness, from_words, gaussians, generator, harness_rows, hexfloat, np_next,
                         np_tanh, same_floats, words)

REF_HEADER = "/root/reference/badmaths.h"


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("dream_rule"))


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    """the same program under AddressSanitizer and UndefinedBehaviorSanitizer: it has its own main, so the runtimes are
    linked into it and nothing is preloaded"""
    return build_harness(tmp_path_factory.mktemp("dream_rule_san"),
                         ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def ask_bits(exe, tmp_path, values, *args):
    path = str(tmp_path / "values.f32")
    np.ascontiguousarray(values, F).tofile(path)
    r = subprocess.run([exe] + [str(a) for a in args] + [path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.array(r.stdout.split(), np.uint64).astype(np.uint32).view(F)


def test_the_header_needs_no_hip_and_is_c_as_well():
    hdr = os.path.join(CSRC, "dream_rule.h")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-x", "c++",
                    hdr], check=True)
    subprocess.run(["gcc", "-std=gnu11", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-x", "c", hdr],
                   check=True)


# ------------------------------------------------------------------ the tanh --

def tanh_inputs():
    """0 and -0, denormals, +-4.97f and both neighbours of each, the infinities and NaN, a sweep of [-6, 6], and what a
    net's outputs look like"""
    g = np.random.default_rng(11)
    tiny = np.array([1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, -1.1754942e-38, 1.17549435e-38], F)
    e = EXTREME
    edge = np.array([e, np.nextafter(e, F(0)), np.nextafter(e, F(10)), -e, np.nextafter(-e, F(0)), np.nextafter(-e, F(-10))], F)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e30, -1e30, 3.4e38, -3.4e38], F)
    sweep = np.linspace(-6.0, 6.0, 100001).astype(F)
    return np.concatenate([special, tiny, edge, sweep, (g.standard_normal(2000) * 2.0).astype(F),
                           g.uniform(-1e3, 1e3, 300).astype(F)])


def check_tanh(exe, tmp_path):
    x = tanh_inputs()
    got = ask_bits(exe, tmp_path, x, "tanh")
    want = np_tanh(x)
    assert same_floats(got, want), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5]
    # what the inputs are there for
    at = {float(v): float(w) for v, w in zip(x[:60], got[:60])}
    assert at[float(EXTREME)] == 1.0 and at[float(-EXTREME)] == -1.0
    assert at[float(np.nextafter(EXTREME, F(10)))] == 1.0 and at[float(np.nextafter(-EXTREME, F(-10)))] == -1.0
    assert 0.9999 < at[float(np.nextafter(EXTREME, F(0)))] < 1.0 and -1.0 < at[float(np.nextafter(-EXTREME, F(0)))] < -0.9999
    assert at[float("inf")] == 1.0 and at[float("-inf")] == -1.0 and at[float(F(1e30))] == 1.0
    assert np.isnan(got[4]) and np.isnan(x[4])
    assert got[0] == 0.0 and not np.signbit(got[0]) and got[1] == 0.0 and np.signbit(got[1])
    assert got[9] == F(1e-45) and got[10] == F(-1e-45)          # a denormal is its own tanh: x * 135135 / 135135
    assert np.all(np.abs(got[~np.isnan(got)]) <= 1.0)
    return x, got


def test_tanh_is_the_restatement_bit_for_bit(harness, tmp_path):
    x, got = check_tanh(harness, tmp_path)
    # and it IS a tanh, to the continued fraction's error (and the clamp's, 1 - tanh(4.97) = 9.6e-5)
    fine = np.isfinite(x)
    assert np.abs(got[fine].astype(np.float64) - np.tanh(x[fine].astype(np.float64))).max() < 1.2e-4


@pytest.mark.parametrize("broken", ["< for <=", "swapped coefficient"])
def test_each_tanh_rule_is_noticed(harness, tmp_path, broken):
    x = tanh_inputs()
    got = ask_bits(harness, tmp_path, x, "tanh")
    wrong = np_tanh(x, broken)
    assert not same_floats(got, wrong), broken
    if broken == "< for <=":   # only the two values +-4.97f themselves can tell
        differ = got.view(np.uint32) != wrong.view(np.uint32)
        assert set(np.abs(x[differ & ~np.isnan(x)]).tolist()) == {float(EXTREME)}


@pytest.mark.skipif(not os.path.exists(REF_HEADER), reason="needs the reference tree (its badmaths.h)")
def test_tanh_is_the_references_fast_tanhf_bit_for_bit(harness, tmp_path):
    """a few lines of C of the test's own that include the reference's header, compiled into the temporary directory"""
    src = tmp_path / "ask_fast_tanhf.c"
    src.write_text('#include <stdio.h>\n#include <string.h>\n#include <math.h>\n#include <stdint.h>\n'
                   '#include <stdbool.h>\ntypedef uint8_t u8;\n'
                   '#define MAX(a, b) ((a) > (b) ? (a) : (b))\n#define MIN(a, b) ((a) < (b) ? (a) : (b))\n'
                   '#include "badmaths.h"\n'
                   'int main(int argc, char **argv) {\n'
                   '  FILE *f = fopen(argv[1], "rb");\n  float x;\n'
                   '  while (f && fread(&x, sizeof x, 1, f) == 1) {\n'
                   '    float y = fast_tanhf(x);\n    unsigned u;\n    memcpy(&u, &y, sizeof u);\n    printf("%u\\n", u);\n  }\n'
                   '  return f ? 0 : 1;\n}\n')
    exe = str(tmp_path / "ask_fast_tanhf")
    subprocess.run(["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-D_GNU_SOURCE", "-I", os.path.dirname(REF_HEADER),
                    str(src), "-o", exe, "-lm"], check=True)
    x = tanh_inputs()
    want = ask_bits(exe, tmp_path, x)
    assert same_floats(ask_bits(harness, tmp_path, x, "tanh"), want)


# ------------------------------------------------------------------ the next input --

def next_pairs():
    g = np.random.default_rng(12)
    a = np.concatenate([g.uniform(-1.0, 1.0, 4000), [1.0, -1.0, 0.0, -0.0, 1e-45, 0.99990004, np.nan]]).astype(F)
    gz = np.concatenate([gaussians(generator(5), 4000), [6.0, -6.0, 0.0, -1.0, 1.0, 1.5259022e-05, 0.5]]).astype(F)
    return a, gz


def check_next(exe, tmp_path):
    a, gz = next_pairs()
    for noise in (1.0, 0.25, 0.0, -0.5, 1.0 / 3.0):
        got = ask_bits(exe, tmp_path, np.stack([a, gz], axis=1), "next", hexfloat(noise))
        assert same_floats(got, np_next(a, noise, gz)), noise
    one = ask_bits(exe, tmp_path, np.stack([a, gz], axis=1), "next", hexfloat(1.0))
    with np.errstate(invalid="ignore"):
        assert same_floats(one, a * (F(1.0) + gz))                 # gstparrot.c:576: noise 1 is exact
    assert same_floats(ask_bits(exe, tmp_path, np.stack([a, gz], axis=1), "next", hexfloat(0.0))[:-1], a[:-1])
    return a, gz, one


def test_next_is_the_restatement_bit_for_bit(harness, tmp_path):
    check_next(harness, tmp_path)


def test_the_fused_looking_form_is_noticed(harness, tmp_path):
    a, gz, one = check_next(harness, tmp_path)
    assert not same_floats(one, np_next(a, 1.0, gz, "a + a * g"))
    third = ask_bits(harness, tmp_path, np.stack([a, gz], axis=1), "next", hexfloat(1.0 / 3.0))
    assert not same_floats(third, np_next(a, 1.0 / 3.0, gz, "a + a * g"))


# ------------------------------------------------------------------ the draw order --

def check_draw_order(exe, tmp_path):
    """one row of 7 outputs over three frames: the draws are the oracle's, one per output in index order, frame after
    frame, and the generator afterwards is the oracle's after 21 values"""
    n, noise = 7, 0.5
    raw = (np.random.default_rng(13).standard_normal((3, n)) * 3.0).astype(F)
    raw[1, 2] = 7.0
    mine = generator(77)
    state = words(mine)[None, :]
    reverse_differs = False
    for t in range(3):
        frame, nxt, state = harness_rows(exe, tmp_path, noise, raw[t:t + 1], state)
        gz = gaussians(mine, n)
        assert same_floats(frame[0], np_tanh(raw[t])) and same_floats(nxt[0], np_next(np_tanh(raw[t]), noise, gz)), t
        reverse_differs |= not same_floats(nxt[0], np_next(np_tanh(raw[t]), noise, gz[::-1]))
        assert np.array_equal(state[0], words(mine)), t
    assert reverse_differs
    # noise 0 draws nothing: the generator is as it was and the next row is the frame
    frame, nxt, after = harness_rows(exe, tmp_path, 0.0, raw[:2], np.stack([state[0], state[0] + np.uint64(1)]))
    assert same_floats(nxt, frame) and np.array_equal(after[0], state[0]) and np.array_equal(after[1], state[0] + np.uint64(1))
    # two rows: each its own generator, the second's draws not the first's
    two = np.stack([words(generator(1)), words(generator(2))])
    _, nxt, after = harness_rows(exe, tmp_path, 1.0, np.stack([raw[0], raw[0]]), two)
    for k in range(2):
        g = from_words(two[k])
        assert same_floats(nxt[k], np_next(np_tanh(raw[0]), 1.0, gaussians(g, n))) and np.array_equal(after[k], words(g))
    assert not same_floats(nxt[0], nxt[1])


def test_the_draws_are_the_oracles_in_index_order(harness, tmp_path):
    check_draw_order(harness, tmp_path)


def test_under_address_and_undefined_behaviour_sanitizers(sanitized, tmp_path):
    """stand-alone: the harness has its own main, the sanitizers' runtimes are linked into it"""
    check_tanh(sanitized, tmp_path)
    check_next(sanitized, tmp_path)
    check_draw_order(sanitized, tmp_path)


# ------------------------------------------------------------------ the call's refusals need no device --

@pytest.fixture(scope="module")
def lib():
    return rc.bind_char(rc.load_amd())


def test_refusals_and_the_early_returns_need_no_device(lib):
    """-1 with nothing written, and 0 for no frames or no sequences, on a machine without a GPU (no compute entry point is
    reached; with a device present the same calls return before they touch it)"""
    net = lib.rnn_new(5, 9, 5, rc.FLAG_STANDARD, 1, None, 4, 1e-3, 0.9, 0.0, rc.RELU)
    uneven = lib.rnn_new(5, 9, 6, rc.FLAG_STANDARD, 1, None, 4, 1e-3, 0.9, 0.0, rc.RELU)
    bottom = lib.rnn_new_with_bottom_layer(7, 5, 9, 5, rc.FLAG_STANDARD, 5, None, 4, 1e-3, 0.9, 0.0, rc.RELU, 0)
    H, n = net.contents.h_size, 3
    g = np.random.default_rng(2)
    first = g.random((n, 6)).astype(F)                      # (rows of 6 floats for 5 inputs)
    frames = np.full(2 * n * 5, 7.0, F)
    nxt = np.full((n, 5), 7.0, F)
    h_in = g.random((n, H)).astype(F)
    h_out = np.full((n, H), 5.0, F)
    seeds = np.array([3, 4, 5], np.uint64)
    rng_in = np.stack([words(generator(int(s) + 10)) for s in seeds])
    rng_out = np.full((n, 4), 9, np.uint64)
    u64p, ctxp = C.POINTER(C.c_uint64), C.POINTER(rc.RandCtx)

    def call(net=net, first=rc.fptr(first), ld=6, n=n, n_frames=2, noise=1.0, seeds=seeds.ctypes.data_as(u64p), rng_in=None,
             h_in=rc.fptr(h_in), h_out=rc.fptr(h_out), segment=0, frames=rc.fptr(frames), nxt=rc.fptr(nxt),
             rng_out=rng_out.ctypes.data_as(ctxp)):
        return lib.rnn_amd_dream_sequences(net, first, ld, n, n_frames, noise, seeds, rng_in, h_in, h_out, segment, frames, nxt,
                                           rng_out)

    assert call(net=None) == -1
    assert call(n=-1) == -1 and call(n_frames=-1) == -1
    assert call(ld=4) == -1
    assert call(net=uneven) == -1                                                      # 5 inputs, 6 outputs
    assert call(net=bottom) == -1                                                      # a bottom layer
    assert call(first=None) == -1 and call(frames=None) == -1
    assert call(seeds=None) == -1 and call(seeds=None, noise=0.25) == -1               # noise and no generator
    assert call(noise=float("nan")) == -1 and call(noise=float("inf")) == -1 and call(noise=float("-inf")) == -1
    assert np.all(frames == 7.0) and np.all(nxt == 7.0) and np.all(h_out == 5.0) and np.all(rng_out == 9)   # nothing written
    # no sequences: 0, and nothing touched
    assert call(n=0) == 0 and call(n=0, first=None, frames=None, seeds=None) == 0
    assert np.all(nxt == 7.0) and np.all(h_out == 5.0) and np.all(rng_out == 9)
    # no frames: 0 at once, no device asked for; next = first, the generators as seeded, the states copied by the host
    assert call(n_frames=0, frames=None) == 0
    assert np.array_equal(nxt, first[:, :5]) and np.array_equal(h_out[:, 1:10], h_in[:, 1:10]) and np.all(frames == 7.0)
    assert np.array_equal(rng_out, np.stack([words(generator(int(s))) for s in seeds]))
    # ... or as handed in, which goes before the seeds; in place
    assert call(n_frames=0, rng_in=rng_in.ctypes.data_as(ctxp)) == 0 and np.array_equal(rng_out, rng_in)
    same_h, same_g = h_in.copy(), rng_in.copy()
    assert call(n_frames=0, seeds=None, rng_in=same_g.ctypes.data_as(ctxp), rng_out=same_g.ctypes.data_as(ctxp),
                h_in=rc.fptr(same_h), h_out=rc.fptr(same_h)) == 0
    assert np.array_equal(same_g, rng_in) and np.array_equal(same_h[:, 1:10], h_in[:, 1:10])
    # noise 0 needs no generator and writes none
    rng_out[:] = 9
    assert call(n_frames=0, noise=0.0, seeds=None) == 0 and np.all(rng_out == 9)
    assert call(n_frames=0, h_out=None, nxt=None, rng_out=None) == 0 and call(n_frames=0, h_in=None, h_out=None) == 0
    # with h_in NULL the start state is the net's hidden row, which only the host has here
    rc.view(net.contents.hidden_layer, H)[1:10] = np.arange(9, dtype=F)
    assert call(n_frames=0, h_in=None) == 0
    assert np.array_equal(h_out[:, 1:10], np.tile(np.arange(9, dtype=F), (n, 1)))
    for x in (bottom, uneven, net):
        lib.rnn_delete_net(x)
