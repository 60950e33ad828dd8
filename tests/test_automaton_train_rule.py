"""What rnnca's trainers are fed and scored against, asked of the rule itself (recur_amd/csrc/automaton_train_rule.h, what
k_automaton_train_rows runs on the device) without a GPU: automaton_train_rule_harness.cpp is compiled with g++ alone and
prints the rows and targets of a block, the momentum of a generation and the refusals of rnn_amd_set_automaton_steps.  The
expected values are tests/automaton_train_cases.py's numpy restatement of gstrnnca.c:669-708 and 726-728 and must be met bit
for bit.  The restatement is then broken one rule at a time, and each broken form must differ on these inputs: the device
tests, which hold the call to the same restatement, would notice that rule being wrong."""
import os
import subprocess

import numpy as np
import pytest

import automaton_train_cases as ac
import recur_ctypes as rc

ROOT = rc.ROOT
CSRC = os.path.join(ROOT, "recur_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "automaton_train_rule_harness.cpp")
CXX = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
F = np.float32


def build(tmp_path_factory, name, extra=()):
    exe = str(tmp_path_factory.mktemp(name) / "automaton_train_rule_harness")
    subprocess.run(CXX + list(extra) + [SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build(tmp_path_factory, "automaton_train_rule")


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    """the same program under AddressSanitizer and UndefinedBehaviorSanitizer: it has its own main, so the runtimes are
    linked into it and nothing is preloaded"""
    return build(tmp_path_factory, "automaton_train_rule_san", ["-O1", "-g", "-fsanitize=address,undefined",
                                                                "-fno-sanitize-recover=all"])


def ask(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_the_header_needs_no_hip_and_is_c_as_well():
    hdr = os.path.join(CSRC, "automaton_train_rule.h")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-x", "c++",
                    hdr], check=True)
    subprocess.run(["gcc", "-std=gnu11", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-x", "c", hdr],
                   check=True)


# ------------------------------------------------------------------ rows and targets --

@pytest.fixture(scope="module")
def cases():
    """(name, grid, T, xy, film), the films with 0, 1, 254 and 255 planted under the trainers and their neighbours"""
    out = []
    for k, (name, g, T, xy) in enumerate(ac.rule_cases()):
        out.append((name, g, T, xy, ac.plant(g, ac.film_of(g, T, 100 + k), xy)))
    return out


def harness_block(exe, directory, g, T, xy, film):
    fpath, xpath = os.path.join(str(directory), "film.u8"), os.path.join(str(directory), "xy.i32")
    np.ascontiguousarray(film, np.uint8).tofile(fpath)
    xy = np.ascontiguousarray(xy, np.int32)
    xy.tofile(xpath)
    n = xy.shape[-2]
    bits = np.array(ask(exe, "block", g.width, g.height, g.edges, g.len_pos, ac.pattern_of(g), T, n, int(xy.ndim == 3), fpath,
                        xpath).split(), np.int64).astype(np.uint32)
    rows = bits[:T * n * g.input_size].reshape(T, n, g.input_size)
    return rows, bits[T * n * g.input_size:].reshape(T, n, 3)


def check_blocks(exe, directory, cases):
    seen = set()
    for name, g, T, xy, film in cases:
        rows, targets = harness_block(exe, directory, g, T, xy, film)
        want_rows, want_targets = ac.np_block(g, film, xy)
        assert np.array_equal(rows, want_rows.view(np.uint32)), name
        assert np.array_equal(targets, want_targets.view(np.uint32)), name
        seen |= set(np.unique(want_targets.view(np.uint32)).tolist())
    for b in ac.PLANTED:      # the planted bytes were scored
        assert ac.np_unit(b).view(np.uint32) in seen, b


def test_rows_and_targets_are_the_restatement_bit_for_bit(harness, tmp_path, cases):
    assert len(cases) == 13 and {(g.width, g.height) for _, g, _, _, _ in cases} == {(3, 3), (5, 4), (16, 12)}
    assert any(len(xy) == 9 and xy.ndim == 2 for _, g, _, xy, _ in cases if g.width == 3)      # a trainer on every cell
    assert any(not g.cs for _, g, _, _, _ in cases)
    check_blocks(harness, tmp_path, cases)


@pytest.mark.parametrize("broken", ac.BROKEN)
def test_each_rule_is_noticed(cases, broken):
    """the restatement with one rule broken differs from the whole one on these very inputs"""
    differ = 0
    for name, g, T, xy, film in cases:
        rows, targets = ac.np_block(g, film, xy)
        brows, btargets = ac.np_block(g, film, xy, broken)
        differ += not (np.array_equal(rows.view(np.uint32), brows.view(np.uint32)) and
                       np.array_equal(targets.view(np.uint32), btargets.view(np.uint32)))
    assert differ >= 1, broken


def test_the_bytes_where_reciprocal_and_division_differ_are_in_the_films(cases):
    """BYTE_TO_UNIT multiplies by the rounded reciprocal of 255; the bytes whose quotient is another float are worked out
    here, and the films hold some of them under a trainer"""
    differ = ac.unit_differs()
    print("bytes whose product with 1.0f / 255.0f is not their quotient by 255:", differ.tolist())
    assert 0 < len(differ) < 256 and 0 not in differ
    hit = 0
    for name, g, T, xy, film in cases:
        pos = ac.per_step(xy, T)
        own = film[1:, :, pos[:, :, 1], pos[:, :, 0]]
        hit += int(np.isin(own, differ).sum())
    assert hit > 0


# ------------------------------------------------------------------ the momentum --

def test_the_momentum_is_the_oracles_soft_start(harness):
    orc = rc.load_oracle()
    for momentum in (0.5, 0.95):
        for soft in (0.0, 1.0, 50.0, 2000.0):
            for gen in (0, 1, 7, 8, 100, 5000, 1000000):
                got = np.array([int(ask(harness, "momentum", gen, float(F(momentum)).hex(), float(F(soft)).hex()))],
                               np.uint32).view(F)[0]
                if soft == 0.0:
                    assert got.view(np.uint32) == F(momentum).view(np.uint32), (momentum, gen)   # the momentum as it is
                    continue
                want = F(orc.orc_momentum_soft_start(float(gen), momentum, soft))
                assert got.view(np.uint32) == want.view(np.uint32), (momentum, soft, gen, got, want)
                assert ac.np_momenta(gen, 1, momentum, soft)[0].view(np.uint32) == want.view(np.uint32)
    assert F(orc.orc_momentum_soft_start(0.0, 0.95, 50.0)) < F(0.95)        # (the soft start does something)


# ------------------------------------------------------------------ the refusals --

REFUSALS = {
    "valid": 0, "valid per step": 0, "valid wrapped": 0, "valid empty C": 0, "valid clamped long offset": 0,
    "valid: outside behind the one list": 0,
    "no set": 1, "no geometry": 1, "no frames": 1, "no xy": 1,
    "no steps": 2, "negative steps": 2,
    "width 0": 3, "height -1": 3, "2^31 cells": 3,
    "len_y -1": 4, "len_c -1": 4, "NULL Y list": 4, "NULL C list": 4,
    "len_pos 1": 5, "len_pos 4": 5,
    "an input too many": 6, "an input too few": 6,
    "two outputs": 7,
    "bottom layer": 8,
    "wrap as long as the grid": 9,
    "no trainers": 10,
    "x is width": 11, "y is height": 11, "x -1": 11, "y -1": 11, "outside in the second step's list": 11,
}


def check_refusals(exe):
    got, texts = {}, {}
    for line in ask(exe, "refusals").splitlines():
        name, rest = line.split("=", 1)
        code, text = rest.split(" ", 1)
        got[name] = int(code)
        texts.setdefault(int(code), set()).add(text)
    assert got == REFUSALS
    assert set(got.values()) == set(range(12))
    assert all(len(t) == 1 for t in texts.values()) and len({next(iter(t)) for t in texts.values()}) == 12   # a text each


def test_every_refusal_and_the_blocks_it_takes(harness):
    check_refusals(harness)


def test_under_address_and_undefined_behaviour_sanitizers(sanitized, tmp_path, cases):
    """stand-alone: the harness has its own main, the sanitizers' runtimes are linked into it"""
    check_blocks(sanitized, tmp_path, cases)
    check_refusals(sanitized)
    assert ask(sanitized, "momentum", 3, float(F(0.5)).hex(), float(F(2.0)).hex()).strip()
