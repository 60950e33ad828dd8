"""The callers either side of the hot path, on their OWN workloads at BASELINE.json's sizes:

* configs[3], the multi-head character model: the batched device generation at hidden 1024 /
  256 streams (and 32 = the 8-GPU shard) with the fixture net's output shape (73 symbols x 50
  heads = 3650 outputs), ADAGRAD, RESQRT, leakage > 0; and the reference's own trainer loop
  (rnn_char_multitext_train / rnn_char_multi_cross_entropy, charmodel-multi-predict.c:234-408)
  against an oracle restatement of that loop.
* configs[4], rnnca: 35 dense inputs, 3 outputs, sigmoid-slope MSE loss ON THE DEVICE
  (gstrnnca.c:701-714) at hidden 2048 / 512 streams / depth 10, and the frame fill
  (gstrnnca.c:805-831): 13,824 forward-only cells per frame.

Tolerance 1e-4 relative (2-norm and max element), generator states and counters bit-exact.
"""
import ctypes as C
import time

import numpy as np
import pytest

import recur_ctypes as rc
import replay
import scenarios as sc
from test_gpu_parity import _load_state

pytestmark = pytest.mark.gpu
RTOL = 1e-4


@pytest.fixture(scope="module")
def amd():
    lib = rc.load_amd()
    assert lib.rnn_amd_device_count() >= 1, "no HIP device: the product has no CPU fallback"
    rc.bind_char(lib)
    return lib


def _sync_oracle_to(o, snap, g=None,
                    keys=("ih_w", "ho_w", "ih_m", "ho_m", "hist", "hidden", "index", "min_error_factor")):
    a = o.arrays()
    for k in keys:
        a[k][:] = snap[k]
    a["generation"][:] = snap["generation"]
    for j in range(o.S):
        r = o.z.contents.rng[j]
        r.a, r.b, r.c, r.d = (int(x) for x in snap["rng"][j])
        if g is not None:
            # the sparse top path reads last generation's h_error where a hidden node is off
            # (recur-nn.c:175-193): the error images are state too
            b = g.nets[j].contents.bptt.contents
            a["err_a"][j] = rc.view(b.h_error, o.I)
            a["err_b"][j] = rc.view(b.i_error, o.I)


def _same_mask(got, want, allowed=4):
    """the zero pattern of the hidden rows (the reference's zero-row skip keys on it): equal,
    except that a pre-activation within rounding of zero may land on either side in a
    different summation order -- at most a handful among a million, each of them tiny"""
    diff = (got != 0) != (want != 0)
    assert diff.sum() <= allowed, "%d hidden values differ in being zero" % diff.sum()
    if diff.any():
        assert max(np.abs(got[diff]).max(), np.abs(want[diff]).max()) < 1e-5


# ------------------------------------------------------------------ configs[3] --

@pytest.mark.parametrize("S", [256, 32])
def test_config3_multi_head_generation_at_size(amd, S):
    """hidden 1024, alphabet 73 x 50 heads (o_size 3652: the wide-output GEMM path, ranged top
    backprop with one range list per stream), ADAGRAD with ballast, RESQRT, leakage 0.1, noise
    on: the ring is warmed on the device, then one generation on both sides from the same state."""
    _multi_head_generation(amd, 73, 50, 1024, S, 20, 0.1, deep=True)


@pytest.mark.parametrize("S", [256, 32])
def test_config3_multi_head_generation_as_one_call(amd, S):
    """rnn_amd_set_multi_step: the multi-head generation with its ADAGRAD update as ONE call -- the weight-delta GEMM carries
    the update out in its epilogue (DdArgs.method 4: recur-nn.c:518-524, `m += d d; w += d rate / sqrt(m)`, both layers, the
    76 rest rows, the zero-delta columns), no optimiser launch: the same generation against the oracle, weights and
    accumulators included."""
    _multi_head_generation(amd, 73, 50, 1024, S, 20, 0.1, deep=True, one_call=True)


def test_text_step_with_adagrad_in_the_delta_gemms_epilogue(amd):
    """rnn_amd_set_char_step with RNN_ADAGRAD at hidden 1024: the same epilogue through the text step (the top layer's delta
    from the chain launch or the split-K planes, not from the hook, which is the momentum rule's)."""
    kw = dict(input_size=42, hidden_size=1024, output_size=42, S=64, D=10, learn_rate=1e-4, seed=5)
    g = sc.AmdBatchedSet(amd, **kw)
    amd.rnn_set_momentum_values(g.net, 50.0)
    text = sc.synthetic_text(8000)
    for i in range(13):
        g.char_step(text, i, rc.ADAGRAD, 0.9)
    o = sc.OracleSet(**kw)
    for attempt in range(4):
        _sync_oracle_to(o, g.snapshot())
        g.char_step(text, 13 + attempt, rc.ADAGRAD, 0.9)
        o.char_step(text, 13 + attempt, rc.ADAGRAD, 0.9)
        sg, so = g.snapshot(), o.snapshot()
        if np.array_equal(sg["hidden"] != 0, so["hidden"] != 0):
            break
        _same_mask(sg["hidden"], so["hidden"])
    else:
        raise AssertionError("no generation without a rounding-level mask flip in 4 attempts")
    replay.check(sg, so, RTOL, keys=["ih_delta", "ho_delta", "ih_w", "ho_w", "ih_m", "ho_m", "hidden", "hist"],
                 exact=("index", "generation"))
    g.close()
    o.close()


@pytest.mark.parametrize("A,NC,H,S,D,leakage", [(128, 11, 256, 40, 6, 0.3), (24, 64, 512, 300, 5, 0.05),
                                                 (100, 3, 128, 7, 4, 0.9), (31, 20, 256, 64, 6, 0.2),
                                                 (130, 3, 128, 7, 4, 0.9), (64, 64, 512, 128, 4, 0.05),
                                                 (64, 64, 2048, 128, 2, 0.05)])
def test_multi_head_generation_with_other_head_shapes(amd, A, NC, H, S, D, leakage):
    """The per-head top-layer kernels at their limits: the widest head (128 symbols), the narrowest they take (24)
    with the most heads (64) and more than 256 streams (two passes of the stream lists), three heads that nearly
    every stream trains all of (leakage 0.9), 31-symbol heads (never aligned to a float4), 130-symbol heads (past the
    128 that a wave holds in registers: the loss kernel's strided form).  The last two: the smallest sets whose output
    layer is k_fwd_wide's nine-stage form (h_size 516; 128 streams x 4096 outputs = 2 x 64 tiles, fwd_plan.h) and its
    33-stage form (h_size 2052)."""
    _multi_head_generation(amd, A, NC, H, S, D, leakage)


@pytest.mark.parametrize("stray_every", [2, 3])
def test_multi_head_generation_with_streams_that_have_no_head_of_their_own(amd, stray_every):
    """A stream whose class is none of the heads (-1, or one past the last) trains no head of its own and makes one
    leak draw MORE than the others.  The noise of the pass after next is generated before that loss's classes are
    known, on the assumption that every stream's class is a head: every `stray_every`-th generation breaks it, and
    the generator states must still be the reference's, bit for bit."""
    _multi_head_generation(amd, 31, 6, 128, 40, 5, 0.3, stray_every=stray_every)


def _multi_head_generation(lib, A, NC, H, S, D, leakage, deep=False, stray_every=0, one_call=False):
    kw = dict(input_size=A, hidden_size=H, output_size=A * NC, S=S, D=D, learn_rate=1e-4, seed=61,
              activation=rc.RESQRT, noise=0.01, flags=rc.FLAG_STANDARD | rc.FLAG_ADAPTIVE_MIN_ERROR)
    g = sc.AmdBatchedSet(lib, **kw)
    lib.rnn_set_momentum_values(g.net, 200.0)  # the ADAGRAD ballast of py-recur-text.c:437-449
    rs = np.random.default_rng(3)

    n_draws = [0]

    def draw():
        cls = rs.integers(0, NC, S).astype(np.int32)
        n_draws[0] += 1
        if stray_every and n_draws[0] % stray_every == 0:
            cls[::5] = -1
            cls[3::7] = NC
        return rs.integers(0, A, S).astype(np.int32), rs.integers(0, A, S).astype(np.int32), cls

    t0 = time.perf_counter()
    n_warm = D + 3
    for _ in range(n_warm):
        hot, nxt, cls = draw()
        if one_call:  # the update in the weight-delta GEMM's epilogue (ADAGRAD: round 6)
            lib.rnn_amd_set_multi_step(g.handle, rc.iptr(hot), rc.iptr(nxt), rc.iptr(cls), A, leakage, rc.ADAGRAD, 0.9)
        else:
            lib.rnn_amd_set_multi_step_deltas(g.handle, rc.iptr(hot), rc.iptr(nxt), rc.iptr(cls), A, leakage, 0)
            lib.rnn_apply_learning(g.net, rc.ADAGRAD, 0.9)
    lib.rnn_amd_synchronize()
    rate = n_warm * S / (time.perf_counter() - t0)
    print("configs[3] multi-head step, %d streams: %.0f stream-timesteps/s (host uploads per step included)"
          % (S, rate))
    snap = g.snapshot()
    o = sc.OracleSet(**kw)
    _sync_oracle_to(o, snap, g)
    hot, nxt, cls = draw()
    g.stats(clear=True)
    if one_call:
        lib.rnn_amd_set_multi_step(g.handle, rc.iptr(hot), rc.iptr(nxt), rc.iptr(cls), A, leakage, rc.ADAGRAD, 0.9)
    else:
        lib.rnn_amd_set_multi_step_deltas(g.handle, rc.iptr(hot), rc.iptr(nxt), rc.iptr(cls), A, leakage, 0)
        lib.rnn_apply_learning(g.net, rc.ADAGRAD, 0.9)
    ranges = (C.c_int * (2 * (NC + 1)))()
    for j in range(S):
        o.orc.orc_advance(o.z, j)
        o.orc.orc_multi_softmax_error(o.z, j, int(hot[j]), int(nxt[j]), int(cls[j]), A, leakage, ranges)
        o.orc.orc_calc_deltas(o.z, j, 1 if j else 0, ranges)
    o.orc.orc_apply_learning(o.z, rc.ADAGRAD, 0.9)
    sg, so = g.snapshot(), o.snapshot()
    # (the adaptive min_error_factor steers the executed depth towards D / 2, recur-nn.c:399-413)
    assert g.stats().bptt_depth_sum == float(so["bptt_depth"].sum()) and (not deep or so["bptt_depth"].mean() >= D / 4)
    _same_mask(sg["hidden"], so["hidden"])
    trained = (np.abs(so["o_error"])[:, :A * NC].reshape(S, NC, A).sum(axis=2) > 0).sum(axis=1)
    assert (trained.min() >= 1 or stray_every) and trained.max() > 1  # the leakage trained foreign heads too
    replay.check(sg, so, RTOL, keys=["ih_delta", "ho_delta", "ih_w", "ho_w", "ih_m", "ho_m", "hidden", "output",
                                     "o_error", "hist", "min_error_factor", "ih_scale"],
                 exact=("index", "generation", "rng"))
    g.close()
    o.close()


@pytest.mark.parametrize("env,node", [
    ("RECUR_AMD_TOP_SPARSE=0 RECUR_AMD_HO_HEADS=0", "test_config3_multi_head_generation_at_size[32]"),
    ("RECUR_AMD_TOP_SPARSE=0 RECUR_AMD_TOP_HEADS=0 RECUR_AMD_HO_HEADS=0", "test_config3_multi_head_generation_at_size[32]"),
    ("RECUR_AMD_FWD_FUSED_ANY=0 RECUR_AMD_KEEP_DELTAS=0 RECUR_AMD_NOISE_AHEAD=1", "test_config3_multi_head_generation_at_size[32]"),
    ("RECUR_AMD_NOISE_AHEAD=0", "test_multi_head_generation_with_streams_that_have_no_head_of_their_own[2]"),
    ("RECUR_AMD_STALE_FROM_PLANES=0", "test_config3_multi_head_generation_at_size[32]"),
    ("RECUR_AMD_EXTRAS_DENSE=0 RECUR_AMD_KEEP_DELTAS=0", "test_config2_classify_generations_with_balanced_training"),
    # (opinion + loss as one call fall back to the two calls UP FRONT when the one-launch top layer is switched off:
    # round 5 aborted here -- the switch was read only by the launch, after the forward pass had run for it)
    ("RECUR_AMD_DENSE_TOP=0", "test_config2_classify_generations_with_balanced_training"),
    ("RECUR_AMD_DENSE_TOP=0", "test_rnnca_generation_with_opinion_and_loss_in_one_call[512-64-6-12]"),
])
def test_callers_generations_with_the_newer_kernels_switched_off(env, node):
    """Every specialised form has the form it replaced behind it: the multi-head top layer per trained head
    (k_top_heads_partial / _combine, k_ho_delta_heads) falls back to one masked GEMM over the whole output row
    (k_top_backprop_heads; taken when the partial products would not fit) and that to the per-stream ranged gathers
    (any range list); the fused forward launch to assemble + GEMM + finalize; kept delta planes to k_delta_finalize; the
    noise generator two passes ahead to one, to none; k_extras_dense to the generic GEMM; the stale entries from the error
    planes to k_err_writeback's images.  The library reads its
    switches once per process, so each combination runs here in a process of its own."""
    import os
    import subprocess
    import sys
    e = dict(os.environ, **dict(kv.split("=") for kv in env.split()))
    path = "%s::%s" % (os.path.abspath(__file__), node)
    r = subprocess.run([sys.executable, "-m", "pytest", path, "-q", "-x", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=e, timeout=900, cwd=os.path.dirname(os.path.abspath(__file__)))
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("method,batch,leakage,noise", [(rc.ADAGRAD, 5, 0.3, 0.0), (rc.WEIGHTED, 1, 0.0, 0.0),
                                                        (rc.NESTEROV, 7, 0.8, 0.02)])
def test_multitext_trainer_loop_matches_oracle(amd, method, batch, leakage, noise):
    """rnn_char_multitext_train + rnn_char_multi_cross_entropy + rnn_char_multitext_spin with
    the reference's signatures (charmodel.h:242-257) on one net of 3 heads, two texts of
    different classes, against the oracle's restatement of text_train (temporal batching,
    apply between loss and deltas, the net's own momentum)."""
    lib = amd
    A, NC, D = 12, 3, 6
    kw = dict(input_size=A, hidden_size=40, output_size=A * NC, S=1, D=D, learn_rate=3e-3, seed=71,
              activation=rc.RESQRT, noise=noise, momentum=0.9)
    g = sc.ApiSet(lib, **kw)
    o = sc.OracleSet(**kw)
    if method == rc.ADAGRAD:
        lib.rnn_set_momentum_values(g.net, 0.5)
        a = o.arrays()
        a["ih_m"][:] = 0.5
        a["ho_m"][:] = 0.5
    rs = np.random.default_rng(5)
    report = rc.CharProgressReport()
    for cls, n in ((1, 120), (2, 77), (0, 2)):
        text = np.ascontiguousarray(rs.integers(0, A, n).astype(np.uint8))
        lib.rnn_char_multitext_train(g.net, rc.u8ptr(text), n, A, cls, leakage, C.byref(report), None, method,
                                     0.123, batch, None, None, None, 0)
        e, h = C.c_float(0), C.c_float(0)
        o.orc.orc_multitext_train(o.z, 0, rc.u8ptr(text), n, A, cls, leakage, method, 0.9, batch, C.byref(e),
                                  C.byref(h))
        assert abs(report.training_error - e.value / (n - 1)) <= 1e-4 * abs(e.value / (n - 1)) + 1e-7
        assert abs(report.training_entropy + h.value / (n - 1)) <= 1e-4 * abs(h.value / (n - 1)) + 1e-7
        assert report.per_second > 0
    sg, so = g.snapshot(), o.snapshot()
    replay.check(sg, so, RTOL, keys=["ih_w", "ho_w", "ih_m", "ho_m", "ih_delta", "ho_delta", "hidden", "hist",
                                     "min_error_factor"], exact=("index", "generation", "rng"))
    # spin: advance + opinion only
    text = np.ascontiguousarray(rs.integers(0, A, 9).astype(np.uint8))
    lib.rnn_char_multitext_spin(g.net, rc.u8ptr(text), 9, None, None, None, 0)
    for i in range(9):
        o.orc.orc_advance(o.z, 0)
        o.orc.orc_one_hot_opinion(o.z, 0, int(text[i]), noise)
    # (checked right here: every one of the symbols is an input, the last one too -- the device text steps wrap
    # at len - 1, and the spin fed text[0] for the last symbol until tools/gpu_stress_multitext.py compared the
    # state at this point; sixty symbols of cross entropy further on the difference had decayed below 1e-4)
    sg, so = g.snapshot(), o.snapshot()
    replay.check(sg, so, RTOL, keys=["hidden", "output", "hist"], exact=("index", "generation", "rng"))
    # per-head cross entropy of a third text
    text = np.ascontiguousarray(rs.integers(0, A, 60).astype(np.uint8))
    ent_g = (C.c_double * NC)(*([0.0] * NC))
    ent_o = (C.c_double * NC)(*([0.0] * NC))
    lib.rnn_char_multi_cross_entropy(g.net, rc.u8ptr(text), 60, A, ent_g, 7)
    o.orc.orc_multi_cross_entropy(o.z, 0, rc.u8ptr(text), 60, A, ent_o, 7)
    for j in range(NC):
        assert abs(ent_g[j] - ent_o[j]) <= 1e-4 * abs(ent_o[j]), (j, ent_g[j], ent_o[j])
        assert 1.0 < ent_o[j] < 8.0
    sg, so = g.snapshot(), o.snapshot()
    replay.check(sg, so, RTOL, keys=["hidden", "output", "hist"], exact=("index", "generation", "rng"))
    g.close()
    o.close()


def test_multi_confab_object_and_line(amd):
    """rnn_char_new_multi_confab / the confabulation line text_train prints when the text
    length hits the period (charmodel-multi-predict.c:74-119, 145-230, 268-280)."""
    lib = amd
    A, NC = 12, 3
    g = sc.ApiSet(lib, input_size=A, hidden_size=24, output_size=A * NC, S=1, D=4, learn_rate=1e-3, seed=9)
    alpha = lib.rnn_char_new_alphabet()
    lib.rnn_char_alphabet_set_flags(alpha, False, False, False)
    for i, ch in enumerate(b"abcdefghijk^"):
        alpha.contents.points[i] = ch
    alpha.contents.len = A
    mc = lib.rnn_char_new_multi_confab(g.net, alpha, NC, 40, 10, ord("^"))
    assert mc and mc.contents.n_classes == NC and mc.contents.char_len == 40 // NC - 1
    assert mc.contents.byte_len == mc.contents.char_len * 6 + 1 and mc.contents.period == 10
    assert not lib.rnn_char_new_multi_confab(g.net, alpha, NC, 3, 10, -1)  # no room
    mc.contents.bias = 0.0
    text = np.ascontiguousarray((np.arange(11) % A).astype(np.uint8))  # len - 1 == 10: the period
    lib.rnn_char_multitext_train(g.net, rc.u8ptr(text), 11, A, 1, 0.0, None, mc, rc.WEIGHTED, 0.9, 4, None,
                                 None, None, 0)
    strings = [mc.contents.strings[i] for i in range(NC)]
    assert all(len(s) == mc.contents.char_len for s in strings)  # one byte per char, caps markers dropped
    assert all(set(s) <= set(b"abcdefghijkABCDEFGHIJK") for s in strings)
    lib.rnn_char_free_multi_confab(mc)
    lib.rnn_char_free_alphabet(alpha)
    g.close()


# ------------------------------------------------------------------ configs[4] --

def _rnnca_inputs(rs, S, n_in=35):
    """35 inputs per cell: 17 luma + 16 chroma neighbours as BYTE_TO_UNIT bytes, 2 position
    values (gstrnnca.c:668-690); byte 0 is a zero input, which the row rule leaves out"""
    x = (rs.integers(0, 256, (S, n_in)) / np.float32(255.0)).astype(np.float32)
    if n_in >= 3:
        x[:, n_in - 2:] = rs.random((S, 2)).astype(np.float32)
    return np.ascontiguousarray(x)


@pytest.mark.parametrize("hidden,S,D,n_in,activation", [(36, 5, 3, 1, rc.RELU), (100, 33, 7, 46, rc.RESQRT),
                                                         (516, 17, 5, 15, rc.RECLIP20), (256, 48, 4, 47, rc.RELU),
                                                         (128, 9, 6, 16, rc.RESQRT),
                                                         # (hidden 512 / 1024: the extras in the one-launch chain's tail --
                                                         # extras_dense_tail -- with whole and with padded 16-stream tiles)
                                                         (512, 48, 7, 33, rc.RESQRT), (512, 33, 5, 46, rc.RELU),
                                                         (1024, 32, 4, 20, rc.RECLIP20),
                                                         # (60 inputs, 64 extra columns: past k_extras_dense, the generic GEMM + k_extras_finalize)
                                                         (64, 9, 4, 60, rc.RELU)])
def test_dense_input_generation_with_other_shapes(amd, hidden, S, D, n_in, activation):
    """k_extras_dense at its edges: 1 to 47 dense inputs (2 to 48 extra columns: the three 16-column tiles full), h_size
    not a multiple of the 16-deep K chunks, fewer (step, stream) rows than a workgroup takes, every activation's row
    rule.  (48 inputs and more take the generic GEMM: the last case here, the fuzzer at others.)"""
    _rnnca_generation(amd, hidden, S, D, n_in=n_in, activation=activation)


@pytest.mark.parametrize("hidden,S,D", [(2048, 512, 10), (64, 20, 4), (512, 2048, 2), (1024, 2048, 2)])
def test_config4_rnnca_training_generation(amd, hidden, S, D):
    """rnnca's maybe_learn (gstrnnca.c:693-740) for every trainer at once: clear deltas, dense
    35-input opinion, sigmoid-slope MSE against the next frame's Y/Cb/Cr ON THE DEVICE,
    accumulating calc_deltas, weighted-momentum update with the soft start.  The reference's
    trainer never advances the ring (effective depth 1); the synthetic driver adds
    rnn_bptt_advance so that depth 10 is exercised.  The sets of 2048: the fewest rows whose
    hidden layer is k_fwd_wide, in its nine- and seventeen-stage forms (i_size 548 and 1060; fwd_plan.h)."""
    _rnnca_generation(amd, hidden, S, D)


@pytest.mark.parametrize("hidden,S,D,n_in", [(2048, 512, 10, 35), (64, 20, 4, 35), (512, 64, 6, 12)])
def test_rnnca_generation_with_opinion_and_loss_in_one_call(amd, hidden, S, D, n_in):
    """rnn_amd_set_opinion_sigmoid_mse: the same generation with the forward pass's end, the output layer, the loss and the
    top layer's backprop in one launch (k_text_top<1>), the delta call finding the backprop done -- from the generic
    GEMM's K slabs (2048: the fused forward declines more than one round of tiles; 64: not a multiple of 32 columns)
    and from the fused forward's plane (512 / 64)."""
    _rnnca_generation(amd, hidden, S, D, n_in=n_in, combined=True)


@pytest.mark.parametrize("hidden,S,D,n_in", [(2048, 512, 10, 35), (64, 20, 4, 35), (1024, 64, 5, 12)])
def test_rnnca_generation_as_one_call(amd, hidden, S, D, n_in):
    """rnn_amd_set_dense_step_sigmoid_mse: clear, opinion, loss, deltas and the update in one call -- the weight-delta
    GEMM then carries out the momentum rule's update in its epilogue where it is the direct kernel (2048 / 512, 1024 /
    64), and rnn_apply_learning's launch follows where it is not (64 / 20)."""
    _rnnca_generation(amd, hidden, S, D, n_in=n_in, combined="step")


@pytest.mark.parametrize("hidden,S,D,n_in,n_out", [(1024, 64, 5, 12, 640), (1024, 32, 5, 20, 1100), (1024, 96, 5, 33, 516)])
def test_one_call_generation_with_a_wide_top_layer(amd, hidden, S, D, n_in, n_out):
    """The fused update's share of the TOP layer (k_delta_direct.h, mode 2: H * O / 4 float4s shared out over the
    launch's workgroups) where a workgroup's share is more than one float4 per thread: hidden 1024 with 640 / 1100
    outputs is 643 / 1105 float4s per workgroup of 512 threads (round 5's epilogue had no loop there: the tail of
    every share kept its old weights and momentum, and fuse_done suppressed the optimiser launch that would have
    updated them).  Every output carries error (the sigmoid loss over all of them), so every weight moves."""
    _rnnca_generation(amd, hidden, S, D, n_in=n_in, combined="step", n_out=n_out)


def _dense_step_sweep():
    rs = np.random.default_rng(707)
    cases = []
    for hidden in (512, 768, 1024, 1536, 2048):
        for _ in range(2):
            cases.append((hidden, 32 * int(rs.integers(1, 4)), int(rs.choice([5, 10])), int(rs.choice([3, 12, 35, 47, 90])),
                          int(rs.choice([3, 8, 64, 200, 900])), int(rs.choice([rc.RELU, rc.RESQRT, rc.RECLIP20]))))
    return cases


@pytest.mark.parametrize("hidden,S,D,n_in,n_out,activation", _dense_step_sweep())
def test_dense_step_shape_sweep(amd, hidden, S, D, n_in, n_out, activation):
    """rnn_amd_set_dense_step_sigmoid_mse over a seeded sweep of shapes either side of the launcher
    predicates of its fused forms (the dense forward's one round of tiles, the one-launch top layer's o_size <= 64, the
    direct weight-delta kernel's rounds / rest rows / K split, the top layer's share of the fused update), one generation
    from the device's state against the oracle."""
    _rnnca_generation(amd, hidden, S, D, n_in=n_in, activation=activation, combined="step", n_out=n_out)


@pytest.mark.parametrize("between", ["nothing", "put_o_error", "host_weights", "mask_differs", "second_opinion"])
def test_what_happens_between_the_one_call_loss_and_the_delta_call(amd, between):
    """rnn_amd_set_opinion_sigmoid_mse / _grouped_softmax leave the top layer's backprop done for the delta call that
    follows (RamdEngine.top_done) -- unless something touched what it was made from: another output error
    (rnn_amd_set_put_o_error), weights edited on the host, other active flags than the loss returned, another forward
    pass.  Two sets with the same seed, one through the one-call form, one through the separate calls, the same
    intruder on both: a backprop that wrongly survived would show in the deltas at once (they differ by rounding
    otherwise: the one-call launch sums the output layer in another order)."""
    lib = amd
    S, D, NIN = 16, 4, 12
    goff, gsize = np.array([0, 3], np.int32), np.array([3, 4], np.int32)
    kw = dict(input_size=NIN, hidden_size=64, output_size=7, S=S, D=D, learn_rate=3e-3, seed=52)
    ga, gb = sc.AmdBatchedSet(lib, **kw), sc.AmdBatchedSet(lib, **kw)
    rs = np.random.default_rng(29)
    for step in range(6):
        x = (rs.standard_normal((S, NIN)) * 0.6).astype(np.float32)
        x2 = (rs.standard_normal((S, NIN)) * 0.6).astype(np.float32)
        targets = np.stack([rs.integers(-1, 3, S), rs.integers(-1, 4, S)], axis=1).astype(np.int32)
        targets[0] = (1, 2)
        err = (rs.standard_normal((S, ga.O)) * 0.1).astype(np.float32)
        err[:, 7:] = 0
        for g, one_call in ((ga, True), (gb, False)):
            trained = np.zeros(S, np.uint8)
            lib.rnn_bptt_clear_deltas(g.net)
            if one_call:
                lib.rnn_amd_set_opinion_grouped_softmax(g.handle, rc.fptr(x), NIN, 2, rc.iptr(goff), rc.iptr(gsize),
                                                        rc.iptr(targets), None, rc.u8ptr(trained))
            else:
                lib.rnn_amd_set_opinion(g.handle, rc.fptr(x), NIN, None)
                lib.rnn_amd_set_grouped_softmax_error(g.handle, 2, rc.iptr(goff), rc.iptr(gsize), rc.iptr(targets), None,
                                                      rc.u8ptr(trained))
            active = trained.copy()
            if between == "put_o_error":
                lib.rnn_amd_set_put_o_error(g.handle, rc.fptr(err), g.O)
            elif between == "host_weights":
                lib.rnn_amd_sync_host(g.net, rc.RNN_AMD_WEIGHTS)
                how = np.ctypeslib.as_array(g.net.contents.ho_weights, shape=(g.net.contents.ho_size,))
                how[8:24] *= np.float32(1.5)
                lib.rnn_amd_host_written(g.net, rc.RNN_AMD_WEIGHTS)
            elif between == "mask_differs":
                active[:] = 1  # every stream, also those the loss left without a target (their error row is zeros)
            elif between == "second_opinion":
                lib.rnn_amd_set_opinion(g.handle, rc.fptr(x2), NIN, None)
            lib.rnn_amd_set_calc_deltas(g.handle, 1, None, rc.u8ptr(active))
            lib.rnn_amd_set_advance(g.handle)
            lib.rnn_apply_learning(g.net, rc.NESTEROV, 0.9)
        sa, sb = ga.snapshot(), gb.snapshot()
        replay.check(sa, sb, 2e-5, keys=["ih_w", "ho_w", "ih_m", "ho_m", "ih_delta", "ho_delta", "hidden", "output", "hist",
                                         "o_error"], exact=("index", "generation"), elementwise=False)
    ga.close()
    gb.close()


def _rnnca_generation(lib, hidden, S, D, n_in=35, activation=None, combined=False, n_out=3):
    kw = dict(input_size=n_in, hidden_size=hidden, output_size=n_out, S=S, D=D, learn_rate=1e-5 if hidden > 1000 else 1e-3,
              seed=81, momentum=0.95)
    if activation is not None:
        kw["activation"] = activation
    g = sc.AmdBatchedSet(lib, **kw)
    rs = np.random.default_rng(11)

    def generation(gpu, orc_set, x, tgt, gen):
        m = lib.rnn_calculate_momentum_soft_start(float(gen), 0.95, 2000.0)
        if gpu is not None:
            lib.rnn_bptt_clear_deltas(gpu.net)
            lib.rnn_amd_set_advance(gpu.handle)
            if combined == "step":  # the whole generation as one call (the update in the delta GEMM's epilogue)
                lib.rnn_amd_set_dense_step_sigmoid_mse(gpu.handle, rc.fptr(x), n_in, rc.fptr(tgt), n_out, n_out, rc.WEIGHTED, m)
            else:
                if combined:
                    lib.rnn_amd_set_opinion_sigmoid_mse(gpu.handle, rc.fptr(x), n_in, rc.fptr(tgt), n_out, n_out)
                else:
                    lib.rnn_amd_set_opinion(gpu.handle, rc.fptr(x), n_in, None)
                    lib.rnn_amd_set_sigmoid_mse_error(gpu.handle, rc.fptr(tgt), n_out, n_out)
                lib.rnn_amd_set_calc_deltas(gpu.handle, 1, None, None)
                lib.rnn_apply_learning(gpu.net, rc.WEIGHTED, m)
        if orc_set is not None:
            oo = orc_set
            oo.orc.orc_clear_deltas(oo.z)
            for j in range(S):
                oo.orc.orc_advance(oo.z, j)
                oo.orc.orc_opinion(oo.z, j, rc.fptr(np.ascontiguousarray(x[j])), 0.0)
                oo.orc.orc_sigmoid_mse_error(oo.z, j, rc.fptr(np.ascontiguousarray(tgt[j])), n_out)
                oo.orc.orc_calc_deltas(oo.z, j, 1, None)
            oo.orc.orc_apply_learning(oo.z, rc.WEIGHTED, m)

    n_warm = D + 2
    t0 = time.perf_counter()
    for gen in range(n_warm):
        generation(g, None, _rnnca_inputs(rs, S, n_in), (rs.integers(0, 256, (S, n_out)) / np.float32(255)).astype(np.float32),
                   gen)
    lib.rnn_amd_synchronize()
    print("configs[4] rnnca training generation, hidden %d, %d cells: %.0f cell-timesteps/s"
          % (hidden, S, n_warm * S / (time.perf_counter() - t0)))
    o = sc.OracleSet(**kw)
    for attempt in range(4):
        # one generation on both sides from the device's state.  Among a million hidden values
        # one may have a pre-activation within rounding of zero; its mask then depends on the
        # summation order and decides whether that unit's top-layer error exists at all, which
        # shows in one column of the deltas.  Such a generation is not a parity case: go on
        # from where the device is and take the next one.
        _sync_oracle_to(o, g.snapshot())
        x = _rnnca_inputs(rs, S, n_in)
        tgt = np.ascontiguousarray((rs.integers(0, 256, (S, n_out)) / np.float32(255)).astype(np.float32))
        generation(g, o, x, tgt, n_warm + attempt)
        sg, so = g.snapshot(), o.snapshot()
        if np.array_equal(sg["hidden"] != 0, so["hidden"] != 0):
            break
        _same_mask(sg["hidden"], so["hidden"])
    else:
        raise AssertionError("no generation without a rounding-level mask flip in 4 attempts")
    assert np.abs(so["o_error"][:, :n_out]).max() > 0 and (so["o_error"][:, n_out:] == 0).all()
    assert (so["output"][:, :n_out] > 0).all() and (so["output"][:, :n_out] < 1).all()  # the sigmoid landed in place
    replay.check(sg, so, RTOL, keys=["ih_delta", "ho_delta", "ih_w", "ho_w", "ih_m", "ho_m", "hidden", "output",
                                     "hist", "min_error_factor", "ih_scale"],
                 exact=("index", "generation"))
    # o_error = slope * (target - answer) CANCELS against the target (gstrnnca.c:701-714): where the answer is within a
    # hundredth of its target an element carries the answer's 1e-6 a hundredfold -- with hundreds of outputs per cell a few
    # of 50,000 elements read 1.2e-4 of themselves under one summation order and 0.9e-4 under another (round 6: the case
    # with 516 outputs through the generic output layer).  Held to the norm bars; the answers element by element above.
    replay.check(sg, so, RTOL, keys=["o_error"], exact=(), elementwise=n_out <= 3)
    g.close()
    o.close()


def test_config4_rnnca_frame_fill_13824_cells(amd):
    """fill_frame (gstrnnca.c:805-831): one forward-only clone per pixel of the 144 x 96 frame
    (gstrnnca.h:14-15), 35 dense inputs each, fast_sigmoid on the three outputs -- as ONE
    batched call per frame at hidden 2048; checked against the oracle on a sample of cells
    and timed."""
    lib = amd
    W, Hh, hidden = 144, 96, 2048
    F = W * Hh
    net = lib.rnn_new(35, hidden, 3, rc.FLAG_OWN_WEIGHTS, 91, None, 0, 0.0, 0.0, 0.0, rc.RELU)
    lib.rnn_randomise_weights_auto(net)
    fl = net.contents.flags & ~(rc.FLAG_OWN_WEIGHTS | rc.FLAG_OWN_BPTT)
    cells = (rc.NetP * F)()
    for k in range(F):
        cells[k] = lib.rnn_clone(net, fl, rc.SUBSEED, None)
    handle = lib.rnn_amd_set_open(cells, F)
    assert handle
    O = net.contents.o_size
    rs = np.random.default_rng(13)
    out = np.zeros((F, O), np.float32)
    frames = 4
    xs = [_rnnca_inputs(rs, F) for _ in range(frames)]
    lib.rnn_amd_set_opinion(handle, rc.fptr(xs[0]), 35, None)  # first touch: allocation, uploads
    lib.rnn_amd_set_sigmoid_outputs(handle, 3, rc.fptr(out))
    first = out.copy()
    t0 = time.perf_counter()
    for f in range(1, frames):
        lib.rnn_amd_set_opinion(handle, rc.fptr(xs[f]), 35, None)
        lib.rnn_amd_set_sigmoid_outputs(handle, 3, rc.fptr(out))
    dt = (time.perf_counter() - t0) / (frames - 1)
    print("configs[4] rnnca frame fill: %d cells at hidden %d in %.2f ms = %.0f frames/s (inputs uploaded and "
          "answers downloaded every frame)" % (F, hidden, dt * 1e3, 1.0 / dt))
    # the oracle on a sample of cells through all the frames (the state is recurrent)
    sample = [0, 1, 143, 144, 7000, F - 1]
    kw = dict(input_size=35, hidden_size=hidden, output_size=3, S=len(sample), D=1, learn_rate=0.0, seed=91)
    o = sc.OracleSet(**kw)
    a = o.arrays()
    lib.rnn_amd_sync_host(net, rc.RNN_AMD_WEIGHTS)
    a["ih_w"][:] = rc.view(net.contents.ih_weights, o.I, o.H)
    a["ho_w"][:] = rc.view(net.contents.ho_weights, o.H, o.O)
    for f in range(frames):
        for q, k in enumerate(sample):
            o.orc.orc_opinion(o.z, q, rc.fptr(np.ascontiguousarray(xs[f][k])), 0.0)
            ans = a["output"][q]
            for i in range(3):
                ans[i] = o.orc.orc_fast_sigmoid(float(ans[i]))
        if f == 0:
            assert rc.rel_err(first[sample, :3], a["output"][:, :3]) < RTOL
    assert rc.rel_err(out[sample, :3], a["output"][:, :3]) < RTOL
    assert rc.max_err(out[sample, :3], a["output"][:, :3]) < RTOL
    assert (out[:, :3] > 0).all() and (out[:, :3] < 1).all()
    hid = np.zeros(o.H, np.float32)
    lib.rnn_amd_sync_host(cells[7000], rc.RNN_AMD_STREAM)
    hid[:] = rc.view(cells[7000].contents.hidden_layer, o.H)
    assert rc.rel_err(hid, a["hidden"][4]) < RTOL
    lib.rnn_amd_set_close(handle)
    for k in range(F):
        lib.rnn_delete_net(cells[k])
    lib.rnn_delete_net(net)
    o.close()


def test_config2_classify_generations_with_balanced_training(amd):
    """BASELINE.json configs[2] (gstclassify: 512 hidden, 128 channels, 2 classes, Nesterov) through
    rnn_amd_classify_generation -- maybe_learn's body (gstclassify.c:2196-2257) with the balanced-training
    draws (2190-2215, 2096-2104) from the prototype's generator -- against the same loop written out over the
    oracle's per-stream calls.  The sample of windows that train, the seen / used counts and the generator
    must be identical; the nets to 1e-4 on the generations without a hidden unit within rounding of zero."""
    lib = rc.bind_classify(amd)
    S, D, NIN = 128, 12, 32
    kw = dict(input_size=NIN, hidden_size=512, output_size=2, S=S, D=D, learn_rate=3e-4, seed=9, momentum=0.9)
    g = sc.AmdBatchedSet(lib, **kw)
    o = sc.OracleSet(**kw)
    goff, gsize = np.array([0], np.int32), np.array([2], np.int32)
    bal = lib.rnn_amd_balanced_new(2, 1.5)
    seen, used = np.zeros(2, np.uint32), np.zeros(2, np.uint32)
    to_unit = np.float32(1.0) / np.float32(float(0xfffffffffffffffe))
    rs = np.random.default_rng(17)
    flags = g.net.contents.flags
    compared = 0
    for gen in range(8):
        x = (rs.standard_normal((S, NIN)) * 0.5).astype(np.float32)
        tg = rs.choice([0, 0, 0, 1, -1], size=(S, 1)).astype(np.int32)  # class 0 three times as common; some unlabelled
        n = lib.rnn_amd_classify_generation(g.handle, rc.fptr(x), NIN, 1, rc.iptr(goff), rc.iptr(gsize), rc.iptr(tg), None,
                                            bal, rc.NESTEROV, 2000.0, 1)
        # ---- the reference's loop on the oracle
        o.orc.orc_clear_deltas(o.z)
        share = np.float32(1.0) / np.float32(np.float32(seen.sum()) + np.float32(1.0))
        train_p = np.power(np.float32(1.0) - seen.astype(np.float32) * share, np.float32(1.5)).astype(np.float32)
        wins, wrong, trained_groups = C.c_int(0), C.c_float(0), 0
        for j in range(S):
            o.orc.orc_opinion(o.z, j, rc.fptr(np.ascontiguousarray(x[j])), 0.0)
            t = int(tg[j, 0])
            eff = np.array([-1], np.int32)
            if 0 <= t < 2:
                seen[t] += 1
                draw = np.float32(np.float32(o.orc.orc_rand64(C.byref(o.z.contents.rng[0]))) * to_unit)
                if train_p[t] > draw:
                    used[t] += 1
                    eff[0] = t
            k = o.orc.orc_grouped_softmax_error(o.z, j, 1, rc.iptr(goff), rc.iptr(gsize), rc.iptr(eff), None,
                                                C.byref(wins), C.byref(wrong))
            if k:
                o.orc.orc_calc_deltas(o.z, j, 1, None)
            trained_groups += k
            o.orc.orc_advance(o.z, j)
        if wrong.value:
            gen0 = float(o.arrays()["generation"][0])
            o.orc.orc_apply_learning(o.z, rc.NESTEROV, o.orc.orc_momentum_soft_start(gen0, 0.9, 2000.0))
        o.orc.orc_condition(o.z, flags)
        # ---- the sample, the counts, the generator: exactly
        assert n == trained_groups
        assert list(bal.contents.seen[:2]) == list(seen) and list(bal.contents.used[:2]) == list(used)
        sg, so = g.snapshot(), o.snapshot()
        assert np.array_equal(sg["rng"][0], so["rng"][0])
        flips = np.argwhere((sg["hidden"] != 0) != (so["hidden"] != 0))
        if len(flips) == 0:
            replay.check(sg, so, RTOL, keys=["ih_w", "ho_w", "ih_m", "ho_m", "ih_delta", "ho_delta", "hidden", "output",
                                             "hist"], exact=("index", "generation"))
            compared += 1
        _load_state(amd, g, so)
    assert compared >= 4 and 0 < used.sum() < seen.sum()  # the draw did leave windows out
    assert used[0] / max(seen[0], 1) < used[1] / max(seen[1], 1)  # ... more of the common class
    lib.rnn_amd_balanced_free(bal)
    g.close()
    o.close()
