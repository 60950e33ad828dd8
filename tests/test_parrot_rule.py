"""recur_amd/csrc/parrot_rule.h -- the loss of parrot's trainer (gstparrot.c:464-477) -- under g++ alone
(-ffp-contract=off) against the numpy float32 restatement of tests/parrot_cases.py, bit for bit: at the edges of the
answer's range and over a seeded sweep.  The restatement is then broken one rule at a time; each broken form must differ
from the header on at least one pair of the sweep, or the comparison could not tell them apart.  The same stand-alone
harness is built once more with -fsanitize=address,undefined and run as it is."""
import os
import subprocess

import numpy as np
import pytest

import dream_cases as dc
import parrot_cases as pc

F = np.float32


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("parrot_rule")
    return pc.build_harness(d), d


def run(exe, directory, mode, first, targets):
    first, targets = np.ascontiguousarray(first, F), np.ascontiguousarray(targets, F)
    src, out = os.path.join(str(directory), "in_" + mode), os.path.join(str(directory), "out_" + mode)
    np.concatenate([first, targets]).tofile(src)
    r = subprocess.run([exe, mode, str(len(first)), src, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    got = {k: np.fromfile(out + "." + k, F) for k in (("answer",) if mode == "raw" else ()) + ("error", "loss")}
    assert all(len(v) == len(first) for v in got.values())
    return got


def test_header_is_stated_once_on_dream_rule():
    """it includes dream_rule.h for the tanh and does not restate the fraction"""
    text = open(os.path.join(dc.CSRC, "parrot_rule.h")).read()
    assert '#include "dream_rule.h"' in text and "135135" not in text
    assert "#include <hip" not in text and "RAMD_HD float parrot_error" in text and "RAMD_HD float parrot_loss" in text


def test_edges_bit_for_bit(harness):
    exe, d = harness
    a, t = pc.edge_pairs()
    got = run(exe, d, "pairs", a, t)
    assert dc.same_floats(got["error"], pc.np_error(a, t))
    assert dc.same_floats(got["loss"], pc.np_loss(a, t))
    one = (np.abs(a) == 1) & np.isfinite(t)
    assert one.any() and np.all(got["error"][one] == 0)          # the clamp's answer has no slope
    nan = np.isnan(a) | np.isnan(t)
    assert np.array_equal(np.isnan(got["error"]), nan)           # a NaN on either side, and nothing else, is a NaN error


def test_outputs_that_are_not_finite(harness):
    """an infinite output is clamped: answer +-1, error exactly 0 for a finite target; a NaN output is NaN in both"""
    exe, d = harness
    raw = np.array([np.inf, -np.inf, np.nan, 4.97, -4.97, np.nextafter(F(4.97), F(0)), np.nextafter(F(4.97), F(9)), 0.0], F)
    t = np.array([0.5, -0.25, 0.5, 1.0, 0.0, 0.5, 0.5, 0.75], F)
    got = run(exe, d, "raw", raw, t)
    ans, err, loss = pc.np_rule(raw, t)
    assert dc.same_floats(got["answer"], ans) and dc.same_floats(got["error"], err) and dc.same_floats(got["loss"], loss)
    assert got["answer"][0] == 1 and got["answer"][1] == -1 and got["error"][0] == 0 and got["error"][1] == 0
    assert np.isnan(got["answer"][2]) and np.isnan(got["error"][2])
    assert got["answer"][3] == 1 and got["answer"][4] == -1 and abs(got["answer"][5]) < 1 and got["answer"][6] == 1
    assert got["answer"][7] == 0 and got["error"][7] == F(0.75)


def test_sweep_bit_for_bit_and_every_broken_form_shows(harness):
    exe, d = harness
    a, t = pc.sweep_pairs()
    assert len(a) == 100000
    got = run(exe, d, "pairs", a, t)
    assert dc.same_floats(got["error"], pc.np_error(a, t))
    assert dc.same_floats(got["loss"], pc.np_loss(a, t))
    for broken in pc.BROKEN:
        differs = int((got["error"].view(np.uint32) != pc.np_error(a, t, broken).view(np.uint32)).sum())
        assert differs > 0, "the sweep cannot tell the rule from `%s`" % broken


def test_harness_under_sanitizers(tmp_path):
    """the header's host build under AddressSanitizer and UBSan: a program of its own, run directly"""
    exe = pc.build_harness(tmp_path, extra=["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])
    a, t = pc.edge_pairs()
    raw = np.concatenate([a, np.array([np.inf, -np.inf, 1e30, -1e30], F)])
    tt = np.concatenate([t, np.zeros(4, F)])
    src, out = str(tmp_path / "in"), str(tmp_path / "out")
    np.concatenate([raw, tt]).tofile(src)
    r = subprocess.run([exe, "raw", str(len(raw)), src, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    ans, err, _ = pc.np_rule(raw, tt)
    assert dc.same_floats(np.fromfile(out + ".answer", F), ans) and dc.same_floats(np.fromfile(out + ".error", F), err)


def test_which_blocks_of_frames_the_many_step_call_takes(harness):
    """parrot_block_refusal, the rule rnn_amd_set_dense_steps_tanh refuses by (it prints the text and aborts): asked of the
    header without a device.  256 inputs, 256 outputs unless said otherwise; the first thing wrong is named."""
    exe, _ = harness

    def ask(have=1, n_steps=3, ld=256, input_size=256, n=256, output_size=256):
        r = subprocess.run([exe, "block"] + [str(v) for v in (have, n_steps, ld, input_size, n, output_size)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        code, text = r.stdout.strip().split(" ", 1)
        return int(code), text

    assert ask() == (0, "a block it takes") and ask(n_steps=1)[0] == 0 and ask(ld=300)[0] == 0
    assert ask(n=3, ld=256)[0] == 0 and ask(input_size=8, n=256, ld=256)[0] == 0 and ask(input_size=8, n=3, output_size=5, ld=8)[0] == 0
    assert ask(have=0) == (1, "no frames") and ask(have=0, n_steps=0)[0] == 1
    assert ask(n_steps=0) == (2, "fewer than one generation") and ask(n_steps=-4)[0] == 2
    assert ask(n=0) == (3, "targets outside the outputs") and ask(n=257)[0] == 3 and ask(n=-1)[0] == 3
    assert ask(ld=255) == (4, "rows too short for a frame") and ask(input_size=8, n=3, output_size=5, ld=7)[0] == 4
    assert ask(input_size=2, n=5, output_size=5, ld=4)[0] == 4 and ask(ld=0)[0] == 4
    # ... and the call refuses by this rule, not by a restatement of it
    text = open(os.path.join(dc.CSRC, "set_train.c")).read()
    assert "parrot_block_refusal(frames != NULL, n_steps, ld, e->sh.input_size, n, e->sh.output_size)" in text
