"""recur_amd/csrc/sigmoid_rule.h -- the loss of rnnca's trainer (gstrnnca.c:701-714) -- under g++ alone
(-ffp-contract=off) against a numpy float32 restatement whose exponential is the oracle's (orc_fast_expf; an argument that
is not finite is a NaN, fast_exp_rule.h's rule), bit for bit: at 0, at the neighbours of the exponential's scaling
threshold and the other arguments tests/loss_edge_cases.py lists, at both infinities and NaN, and over a seeded sweep.
The restatement is then broken one rule at a time; each broken form must differ from the header somewhere, or the
comparison could not tell them apart.  The same stand-alone harness is built once more with
-fsanitize=address,undefined and run as it is."""
import os
import subprocess

import numpy as np
import pytest

import dream_cases as dc
import loss_edge_cases as lec
import recur_ctypes as rc

F = np.float32
SRC = os.path.join(rc.ROOT, "tests", "sigmoid_rule_harness.cpp")
BROKEN = ("(1 - a) * diff", "slope * (a - target)", "a - a * a", "fused a * (1 - a) * diff")


def build_harness(directory, extra=()):
    exe = os.path.join(str(directory), "sigmoid_rule_harness" + ("_san" if extra else ""))
    subprocess.run(dc.CXX + list(extra) + [SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("sigmoid_rule")
    return build_harness(d), d


def run(exe, directory, raw, targets, tag="x"):
    raw, targets = np.ascontiguousarray(raw, F), np.ascontiguousarray(targets, F)
    src, out = os.path.join(str(directory), "in_" + tag), os.path.join(str(directory), "out_" + tag)
    np.concatenate([raw, targets]).tofile(src)
    r = subprocess.run([exe, str(len(raw)), src, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    got = {k: np.fromfile(out + "." + k, F) for k in ("answer", "error", "loss")}
    assert all(len(v) == len(raw) for v in got.values())
    return got


def oracle_exp(x):
    """the oracle's fast_expf of every finite argument (its loop is badmaths.h's and does not end on an infinity); NaN for
    the others"""
    orc = rc.load_oracle()
    return np.array([orc.orc_fast_expf(float(v)) if np.isfinite(v) else np.nan for v in np.asarray(x, F)], F)


def np_rule(raw, target, broken=None):
    """-> (answer, error, loss): every float32 operation rounded once, none fused"""
    x, t = np.asarray(raw, F), np.asarray(target, F)
    with np.errstate(all="ignore"):
        arg = ((-x).astype(F) * F(1.0)).astype(F)
        a = (F(1.0) / (F(1.0) + oracle_exp(arg)).astype(F)).astype(F)
        diff = (t - a).astype(F)
        loss = (diff * diff).astype(F)
        if broken == "(1 - a) * diff":
            return a, ((F(1.0) - a).astype(F) * diff).astype(F), loss
        if broken == "a - a * a":
            return a, ((a - (a * a).astype(F)).astype(F) * diff).astype(F), loss
        if broken == "fused a * (1 - a) * diff":  # the product of three in float64, rounded once
            a64 = a.astype(np.float64)
            return a, (a64 * (1.0 - a64) * (t.astype(np.float64) - a64)).astype(F), loss
        slope = (a * (F(1.0) - a).astype(F)).astype(F)
        if broken == "slope * (a - target)":
            return a, (slope * (a - t).astype(F)).astype(F), loss
        assert broken is None, broken
        return a, (slope * diff).astype(F), loss


def edge_pairs():
    """every argument of loss_edge_cases.sigmoid_arguments (0, -0, the neighbours of +-0.2 where the exponential's scaling
    starts, up to +-1e4), denormals, both infinities and NaN x targets in {0, 1, 0.5, a byte's level, NaN}"""
    x = np.concatenate([lec.sigmoid_arguments(), np.array([1e-45, -1e-45, 1e-39, -1e-39, np.inf, -np.inf, np.nan], F)])
    t = np.array([0.0, 1.0, 0.5, 200.0 / 255.0, np.nan], F)
    xx, tt = np.meshgrid(x, t, indexing="ij")
    return xx.ravel().copy(), tt.ravel().copy()


def test_header_is_stated_once_on_fast_exp_rule():
    text = open(os.path.join(dc.CSRC, "sigmoid_rule.h")).read()
    assert '#include "fast_exp_rule.h"' in text and "#include <hip" not in text
    for f in ("sigmoid_answer", "sigmoid_error", "sigmoid_loss"):
        assert "RAMD_HD float %s(" % f in text
    # ... and the loss kernels call it instead of restating it: the sigmoid's division stands in none of them
    kernels = open(os.path.join(dc.CSRC, "kernels_loss.hip")).read()
    assert '#include "sigmoid_rule.h"' in kernels and "1.0f / (1.0f +" not in kernels and kernels.count("sigmoid_answer(") == 4


def test_edges_bit_for_bit(harness):
    exe, d = harness
    x, t = edge_pairs()
    assert (x == 0).any() and np.isposinf(x).any() and np.isneginf(x).any() and np.isnan(x).any()
    got = run(exe, d, x, t, "edges")
    ans, err, loss = np_rule(x, t)
    assert dc.same_floats(got["answer"], ans) and dc.same_floats(got["error"], err) and dc.same_floats(got["loss"], loss)
    # an output that is not finite has a NaN answer and a NaN error (fast_exp_rule.h), and nothing else has
    assert np.array_equal(np.isnan(got["answer"]), ~np.isfinite(x))
    assert np.array_equal(np.isnan(got["error"]), ~np.isfinite(x) | np.isnan(t))
    zero = (x == 0) & (t == 1)
    assert zero.any() and np.all(got["answer"][zero] == F(0.5)) and np.all(got["error"][zero] == F(0.125))
    assert np.all(got["loss"][zero] == F(0.25))


def test_sweep_bit_for_bit_and_every_broken_form_shows(harness):
    exe, d = harness
    rs = np.random.default_rng(4321)
    x = np.concatenate([(rs.standard_normal(20000) * 3.0).astype(F), edge_pairs()[0]])
    t = np.concatenate([rs.uniform(0.0, 1.0, 20000).astype(F), edge_pairs()[1]])
    got = run(exe, d, x, t, "sweep")
    ans, err, loss = np_rule(x, t)
    assert dc.same_floats(got["answer"], ans) and dc.same_floats(got["error"], err) and dc.same_floats(got["loss"], loss)
    for broken in BROKEN:
        b_ans, b_err, _ = np_rule(x, t, broken)
        differs = int((~(dc_same(got["answer"], b_ans) & dc_same(got["error"], b_err))).sum())
        assert differs > 0, "the sweep cannot tell the rule from `%s`" % broken


def dc_same(a, b):
    """elementwise: the same bits, any NaN being as good as another"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def test_harness_under_sanitizers(tmp_path):
    """the header's host build under AddressSanitizer and UBSan: a program of its own, run directly"""
    exe = build_harness(tmp_path, extra=["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])
    x, t = edge_pairs()
    got = run(exe, tmp_path, x, t, "san")
    ans, err, loss = np_rule(x, t)
    assert dc.same_floats(got["answer"], ans) and dc.same_floats(got["error"], err) and dc.same_floats(got["loss"], loss)
