"""The soft clip on the top layer's error sum (recur-nn.c:719-721) in EVERY form of the top layer's backward pass.

The clip is stated once (top_clip, k_common.h) and used by five forms: k_top_backprop (no ranges), k_top_backprop_ranged
with its own tail (one workgroup per stream) or k_top_backprop_scale behind it (a stream's rows shared out), the
multi-head loss's one GEMM over heads (k_top_backprop_heads + k_top_backprop_scale) and its per-trained-head form
(k_top_heads_partial + k_top_heads_combine), and the text step's two top launches (k_text_top, k_text_top2).  Each case
makes EVERY stream's error sum exceed the threshold -- asserted on the oracle's own arrays, so a case that stops
clipping fails -- and compares one call against the oracle from the same state: ih_delta, ho_delta, ih_scale,
min_error_factor at 1e-4, the executed depth equal.  Element by element from 1e-1 of an array's largest element up,
the hot regime's floor (replay.check: clipped streams are that regime)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import recur_ctypes as rc
import replay
import scenarios as sc
from test_gpu_callers import RTOL, _same_mask, _sync_oracle_to

pytestmark = pytest.mark.gpu
KEYS = ["ih_delta", "ho_delta", "ih_scale", "min_error_factor"]


@pytest.fixture(scope="module")
def amd():
    lib = rc.load_amd()
    assert lib.rnn_amd_device_count() >= 1, "no HIP device: the product has no CPU fallback"
    rc.bind_char(lib)
    return lib


def _assert_hot(o, what):
    """on the oracle's own arrays: every stream's sum of |e| is over h_size * MAX_TOP_ERROR_FACTOR and was scaled down"""
    a = o.arrays()
    raw, scaled = a["top_error_raw"], a["top_error_scaled"]
    print("%s: smallest top_error_raw / (2 h_size) = %.3g over %d streams" % (what, float(raw.min()) / (2 * o.H), o.S))
    assert (raw > 2 * o.H).all(), "%s: %d streams are not clipped" % (what, int((raw <= 2 * o.H).sum()))
    assert (scaled < raw).all()


def _compare(g, o, what):
    sg, so = g.snapshot(), o.snapshot()
    _assert_hot(o, what)
    assert g.stats().bptt_depth_sum == float(so["bptt_depth"].sum())
    replay.check(sg, so, RTOL, keys=KEYS, exact=("index", "generation"), elem_floor=1e-1)


def _scale_ho_w(lib, g, factor):
    g.sync()
    rc.view(g.net.contents.ho_weights, g.H, g.O)[:] *= np.float32(factor)
    lib.rnn_amd_host_written(g.net, rc.RNN_AMD_WEIGHTS)


# ------------------------------------------------- rnn_amd_set_put_o_error + rnn_amd_set_calc_deltas --

def _dense_rows(rs, S, n_in, n_out, cols, sigma):
    """dense input rows (half of the values zero) and error rows: N(0, sigma) in `cols`, zero elsewhere"""
    X = (rs.standard_normal((S, n_in)) * (rs.random((S, n_in)) < 0.5)).astype(np.float32)
    E = np.zeros((S, n_out), np.float32)
    E[:, cols] = rs.standard_normal((S, len(cols))) * sigma
    return np.ascontiguousarray(X), np.ascontiguousarray(E)


@pytest.mark.parametrize("form,hidden,S,D,sigma", [("plain", 40, 8, 4, 20.0), ("ranged_shared_out", 40, 8, 4, 20.0),
                                                   ("ranged_one_workgroup", 24, 1040, 2, 80.0)])
def test_the_clip_with_caller_written_error_rows(amd, form, hidden, S, D, sigma):
    """plain: no ranges, k_top_backprop.  ranged_shared_out: the range list (4, 8), (16, 4) with 8 streams: their rows go
    to 16 workgroups each (calc_plan.h: top_nb) and k_top_backprop_scale clips.  ranged_one_workgroup: more than 1024
    streams, one workgroup per stream and the kernel's own tail.  The error rows are drawn N(0, sigma): a hidden row's
    error is then ~ 0.2 sigma sqrt(columns), and at hidden 40 some twenty live rows of sigma 20 sum to 2 to 4 times
    2 h_size in every stream (the oracle run on its own); the least of 1040 streams with a dozen live rows each needs
    sigma 80 for that.  Relu leaves about half of the hidden values zero, so the ranged forms meet stale entries; the
    calls before the compared one (D + 1 of them, with the update between) leave those entries and fill the ring."""
    lib = amd
    kw = dict(input_size=20, hidden_size=hidden, output_size=24, S=S, D=D, learn_rate=1e-4, seed=14)
    ranged = form != "plain"
    cols = list(range(4, 12)) + list(range(16, 20)) if ranged else list(range(24))
    ranges = (rc.ErrorRange * 3)((4, 8), (16, 4), (-1, 0)) if ranged else None
    oranges = rc.iptr(np.array([4, 8, 16, 4, -1, 0], np.int32)) if ranged else None
    rs = np.random.default_rng(31)
    g = sc.AmdBatchedSet(lib, **kw)

    def device_call(X, E):
        lib.rnn_amd_set_advance(g.handle)
        lib.rnn_amd_set_opinion(g.handle, rc.fptr(X), X.shape[1], None)
        lib.rnn_amd_set_put_o_error(g.handle, rc.fptr(E), E.shape[1])
        lib.rnn_amd_set_calc_deltas(g.handle, 0, ranges, None)

    for _ in range(D + 1):
        device_call(*_dense_rows(rs, S, 20, g.O, cols, sigma))
        lib.rnn_apply_learning(g.net, rc.WEIGHTED, 0.9)
    o = sc.OracleSet(**kw)
    _sync_oracle_to(o, g.snapshot(), g)
    g.stats(clear=True)
    X, E = _dense_rows(rs, S, 20, g.O, cols, sigma)
    device_call(X, E)
    a = o.arrays()
    for j in range(S):
        o.orc.orc_advance(o.z, j)
        o.orc.orc_opinion(o.z, j, rc.fptr(X[j]), 0.0)
        a["o_error"][j, :] = E[j]
        o.orc.orc_calc_deltas(o.z, j, 1 if j else 0, oranges)
    if ranged:
        assert (a["hidden"][:, 1:hidden + 1] == 0).any(), "no hidden value is zero: no stale entry in play"
    _compare(g, o, form)
    g.close()
    o.close()


# ------------------------------------------------------------------- the multi-head loss's two forms --

# W_ho is multiplied by this before the compared generation: the smallest power of two that clips every stream of it.
# The oracle's smallest top_error_raw / (2 h_size) over the 40 streams is then 1.92 (0.87 at 32); the test prints it.
MULTI_HEAD_SCALE = 64.0


def test_the_clip_per_trained_head(amd):
    """test_gpu_callers' multi-head sequence (alphabet 31, 6 heads, hidden 128, 40 streams, depth 5, leakage 0.3) with
    W_ho scaled up on the host in front of the compared generation.  With the library's defaults this is
    k_top_heads_partial + k_top_heads_combine; the test below runs it once more as one GEMM over heads."""
    lib = amd
    A, NC, H, S, D, leakage = 31, 6, 128, 40, 5, 0.3
    kw = dict(input_size=A, hidden_size=H, output_size=A * NC, S=S, D=D, learn_rate=1e-4, seed=61,
              activation=rc.RESQRT, noise=0.01, flags=rc.FLAG_STANDARD | rc.FLAG_ADAPTIVE_MIN_ERROR)
    g = sc.AmdBatchedSet(lib, **kw)
    lib.rnn_set_momentum_values(g.net, 200.0)
    rs = np.random.default_rng(3)

    def draw():
        return (rs.integers(0, A, S).astype(np.int32), rs.integers(0, A, S).astype(np.int32),
                rs.integers(0, NC, S).astype(np.int32))

    for _ in range(D + 3):
        hot, nxt, cls = draw()
        lib.rnn_amd_set_multi_step_deltas(g.handle, rc.iptr(hot), rc.iptr(nxt), rc.iptr(cls), A, leakage, 0)
        lib.rnn_apply_learning(g.net, rc.ADAGRAD, 0.9)
    _scale_ho_w(lib, g, MULTI_HEAD_SCALE)
    o = sc.OracleSet(**kw)
    _sync_oracle_to(o, g.snapshot(), g)
    hot, nxt, cls = draw()
    g.stats(clear=True)
    lib.rnn_amd_set_multi_step_deltas(g.handle, rc.iptr(hot), rc.iptr(nxt), rc.iptr(cls), A, leakage, 0)
    ranges = (C.c_int * (2 * (NC + 1)))()
    for j in range(S):
        o.orc.orc_advance(o.z, j)
        o.orc.orc_multi_softmax_error(o.z, j, int(hot[j]), int(nxt[j]), int(cls[j]), A, leakage, ranges)
        o.orc.orc_calc_deltas(o.z, j, 1 if j else 0, ranges)
    _same_mask(g.snapshot()["hidden"], o.snapshot()["hidden"])
    _compare(g, o, "multi-head, W_ho x %g" % MULTI_HEAD_SCALE)
    g.close()
    o.close()


def test_the_clip_in_one_gemm_over_heads():
    """The same generation with the per-head kernels switched off: k_top_backprop_heads and k_top_backprop_scale's clip.
    The library reads its switches once per process, so the forced form runs in a process of its own."""
    e = dict(os.environ, RECUR_AMD_TOP_SPARSE="0", RECUR_AMD_HO_HEADS="0")
    path = "%s::%s" % (os.path.abspath(__file__), "test_the_clip_per_trained_head")
    r = subprocess.run([sys.executable, "-m", "pytest", path, "-q", "-x", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=e, timeout=300, cwd=os.path.dirname(os.path.abspath(__file__)))
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


# ----------------------------------------------------------------------- the text step's top launches --

# (kernel, alphabet, hidden, streams, depth, the factor on W_ho).  Which launch a shape gets is ramd_launch_text_top's
# rule (kernels_loss.hip): k_text_top2 where o_size is a multiple of 4 up to 64 and h_size <= 1088 -- which the text
# model's 42 symbols are at hidden 64 AND at hidden 1024 -- else k_text_top.  So the hidden-64 case has 70 symbols
# (o_size 72: k_text_top) and the hidden-1024 case the usual 42 (k_text_top2).  The factors: the smallest powers of
# two that clip every stream of the compared generation -- the oracle's smallest top_error_raw / (2 h_size) is then
# 1.92 (0.95 at half the factor) and 1.36 (0.66).
TEXT_CASES = [("k_text_top", 70, 64, 8, 4, 64.0), ("k_text_top2", 42, 1024, 32, 4, 128.0)]


@pytest.mark.parametrize("kernel,alphabet,hidden,S,D,factor", TEXT_CASES)
def test_the_clip_in_the_text_steps_top_launch(amd, kernel, alphabet, hidden, S, D, factor):
    lib = amd
    kw = dict(input_size=alphabet, hidden_size=hidden, output_size=alphabet, S=S, D=D, learn_rate=1e-4, seed=5)
    text = sc.synthetic_text(4000, alphabet=alphabet)
    g = sc.AmdBatchedSet(lib, **kw)
    for i in range(D + 1):
        g.char_step(text, i, rc.WEIGHTED, 0.9)
    _scale_ho_w(lib, g, factor)
    o = sc.OracleSet(**kw)
    _sync_oracle_to(o, g.snapshot())
    g.stats(clear=True)
    g.char_step(text, D + 1, rc.WEIGHTED, 0.9)
    o.char_step(text, D + 1, rc.WEIGHTED, 0.9)
    _compare(g, o, "%s, W_ho x %g" % (kernel, factor))
    g.close()
    o.close()
