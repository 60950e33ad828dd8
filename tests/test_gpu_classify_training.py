"""Gstclassify's trainer on the device (gstclassify.c: train_channel 2070-2127, maybe_learn 2180-2257):
rnn_amd_set_classify_steps, rnn_amd_classify_generations, the update gate the loss kernels write and k_apply reads, and
tools/classify_train_amd -B.

  1. the block is the loop, bit for bit: one call against rnn_amd_classify_generation(..., exact_gate 1) per window, twin
     sets held equal in every array, generator, ring index, generation counter and statistic, the statistics cleared first;
  2. the gate script on a written saturated net (tests/classify_train_cases.py): open, closed, unlabelled, open, closed,
     against the oracle twin at the project's parity bar; a closed generation leaves weights and momentum bit for bit and
     the delta arrays hold the loop's sums -- once at a shape whose delta call leaves planes (asked of calc_plan.h);
  3. one block from the device's state against the oracle twin at the bar, `correct` and `count` exact;
  4. a net outside the set is left alone and the deferred state after the call is the loop's;
  5. tools/classify_train_amd -B 1 and -B 16 write the same net, byte for byte;
  6. the block buffer the three block trainers share on an engine: parrot's block, a larger block of windows, parrot's again.
tests/test_classify_train_cases_cpu.py shows on the oracle alone that these cases can notice a failure."""
import os
import subprocess

import numpy as np
import pytest

import classify_train_cases as cc
import recur_ctypes as rc
import replay
import scenarios as sc
import test_calc_plan as calc
from recur_amd.drivers import train_frames, train_windows
from test_gpu_callers import _same_mask, _sync_oracle_to

pytestmark = pytest.mark.gpu
F = np.float32
RTOL = cc.PARITY_BAR
N_IN = 10
FLAGS = rc.FLAG_STANDARD | rc.FLAG_ADAPTIVE_MIN_ERROR      # the sets' default, handed to orc_condition


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("classify_plans") / "calc_plan_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", calc.CSRC, "-I", os.path.join(rc.ROOT, "include"),
                    os.path.join(rc.ROOT, "tests", "calc_plan_harness.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def amd():
    lib = rc.load_amd()
    assert lib.rnn_amd_device_count() >= 1, "no HIP device: the product has no CPU fallback"
    rc.bind_char(lib)
    return rc.bind_classify(lib)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


def hold_twins(ga, gb, what):
    """every array of the two sets' snapshots equal bit for bit -- weights, momentums, deltas, hidden rows, rings, outputs,
    error rows, ring indices, generations and generators -- and the statistics"""
    sa, sb = ga.snapshot(), gb.snapshot()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]) if sa[k].dtype.kind != "f" else same(sa[k], sb[k]), "%s: %s differs" % (what, k)
    ta, tb = ga.stats(), gb.stats()
    for field in ("error", "count", "entropy", "correct"):
        a, b = getattr(ta, field), getattr(tb, field)
        assert np.array([a]).tobytes() == np.array([b]).tobytes(), "%s: statistic %s: %r, %r" % (what, field, a, b)
    return sa


def set_kw(n, hidden, D, groups, noise=0.0, **more):
    kw = dict(input_size=N_IN, hidden_size=hidden, output_size=groups[2], S=n, D=D, seed=71, momentum=cc.MOMENTUM, noise=noise,
              learn_rate=1e-3)
    kw.update(more)
    return kw


def twins(lib, kw, count=2, style=rc.NESTEROV):
    out = [sc.AmdBatchedSet(lib, **kw) for _ in range(count)]
    for gs in out:
        if style == rc.ADAGRAD:      # (its accumulators start above zero, as a caller's would: 0 / sqrt(0) is not a step)
            lib.rnn_set_momentum_values(gs.net, 0.1)
        gs.stats(clear=True)
    return out


def weights_of(groups, seed):
    return np.random.default_rng(seed).uniform(0.25, 2.0, groups[2]).astype(F)


# ------------------------------------------------------------------ 1. the block is the loop --

STYLES = (rc.NESTEROV, rc.WEIGHTED, rc.ADAGRAD)
GROUPS = (cc.ONE_OF_2, cc.GAP, cc.WIDE)
# (name, T, channels, hidden, depth, groups, style, error_weight, soft start, row stride, the generations without a label)
BLOCKS = [("T %d, %d channels" % (T, n), T, n, (24, 99, 512)[(k + k // 3) % 3], (1, 12)[k % 2], GROUPS[k % 3], STYLES[k % 3],
           k % 2 == 1, (cc.SOFT_START, 3.0)[(k // 2) % 2], N_IN + (0, 3)[k % 2], (2,) if T == 5 and k % 2 == 0 else ())
          for k, (T, n) in enumerate((T, n) for T in (1, 5) for n in (1, 3, 4, 64, 130))]
BLOCKS += [("512 hidden, 128 channels, one-launch top", 5, 128, 512, 12, cc.ONE_OF_2, rc.NESTEROV, False, cc.SOFT_START, N_IN, ()),
           ("512 hidden, 130 channels, the separate kernel", 5, 130, 512, 12, cc.ONE_OF_2, rc.NESTEROV, False, cc.SOFT_START, N_IN, ()),
           ("hidden 99, 3 channels, the separate kernel", 5, 3, 99, 12, cc.WIDE, rc.NESTEROV, True, cc.SOFT_START, N_IN, (0,)),
           ("every generation without a label", 2, 4, 24, 3, cc.GAP, rc.NESTEROV, False, cc.SOFT_START, N_IN, (0, 1))]


@pytest.mark.parametrize("c", BLOCKS, ids=lambda c: c[0])
def test_the_block_is_the_loop_bit_for_bit(amd, c):
    lib = amd
    name, T, n, hidden, D, groups, style, weighted, soft, ld, silent = c
    ga, gb = twins(lib, set_kw(n, hidden, D, groups), style=style)
    x, tg = cc.block_of(T, n, N_IN, groups, [T, n, hidden], ld=ld, silent=silent)
    w = weights_of(groups, 3) if weighted else None
    trained = train_windows(lib, ga, x, tg, groups[0], groups[1], error_weight=w, learning_style=style, soft_start=soft)
    assert trained == cc.run_loop(lib, gb, x, tg, groups, weight=w, style=style, soft=soft)
    snap = hold_twins(ga, gb, name)
    masks, active, gen = cc.np_decisions(tg, groups[1])
    assert np.array_equal(snap["generation"], gen), "generation++ per active stream"
    st = ga.stats()
    assert st.count == trained and (trained > 0) == bool(active.any())
    if trained:
        assert st.error > 0 and np.abs(snap["ih_delta"]).max() > 0
    ga.close()
    gb.close()


def test_two_chained_blocks_are_one(amd):
    lib, groups, n = amd, cc.GAP, 7
    ga, gb, gc = twins(lib, set_kw(n, 99, 4, groups), 3)
    x, tg = cc.block_of(5, n, N_IN, groups, 81, silent=(1,))
    train_windows(lib, ga, x, tg, groups[0], groups[1])
    train_windows(lib, gb, x[:2], tg[:2], groups[0], groups[1])
    train_windows(lib, gb, x[2:], tg[2:], groups[0], groups[1])
    cc.run_loop(lib, gc, x, tg, groups)
    hold_twins(ga, gb, "2 + 3")
    hold_twins(ga, gc, "the loop")
    for gs in (ga, gb, gc):
        gs.close()


def test_conditioning_is_rnn_condition_net_in_the_loop(amd):
    """the net's conditioning flags on (scale and zero), nine generations from generation 0: the scale interval
    (generation % 8 == 0) and the zero interval (== 2) are both crossed; without `condition` the block differs"""
    lib, groups, n, T = amd, cc.ONE_OF_2, 7, 9
    flags = rc.FLAG_STANDARD | rc.FLAG_ADAPTIVE_MIN_ERROR | rc.COND_USE_SCALE | rc.COND_USE_ZERO
    ga, gb, gc = twins(lib, set_kw(n, 64, 4, groups, flags=flags), 3)
    x, tg = cc.block_of(T, n, N_IN, groups, 82, unlabelled=0.0)
    train_windows(lib, ga, x, tg, groups[0], groups[1], condition=True)
    cc.run_loop(lib, gb, x, tg, groups)
    train_windows(lib, gc, x, tg, groups[0], groups[1], condition=False)
    hold_twins(ga, gb, "conditioned")
    assert int(ga.snapshot()["generation"][0]) == T
    assert not same(ga.snapshot()["ih_w"], gc.snapshot()["ih_w"]), "the conditioning left no trace: the case shows nothing"
    for gs in (ga, gb, gc):
        gs.close()


@pytest.mark.parametrize("flags,route", [(rc.FLAG_STANDARD | rc.FLAG_ADAPTIVE_MIN_ERROR, "draws ahead"),
                                         (rc.FLAG_STANDARD | rc.FLAG_ADAPTIVE_MIN_ERROR | rc.COND_USE_RAND, "the loop: random damage")])
def test_balanced_training_through_classify_generations(amd, flags, route):
    lib, groups, n, T = amd, cc.GAP, 20, 8
    ga, gb = twins(lib, set_kw(n, 24, 3, groups, flags=flags))
    x, tg = cc.block_of(T, n, N_IN, groups, 83)
    tg[:, :, 0] = np.where(tg[:, :, 0] == 1, 0, tg[:, :, 0])      # (class 0 of the first group is the common one)
    ba, bb = lib.rnn_amd_balanced_new(groups[2], 1.5), lib.rnn_amd_balanced_new(groups[2], 1.5)
    trained = train_windows(lib, ga, x, tg, groups[0], groups[1], balance=ba)
    assert trained == cc.run_loop(lib, gb, x, tg, groups, balance=bb)
    hold_twins(ga, gb, route)
    seen, used = list(ba.contents.seen[:groups[2]]), list(ba.contents.used[:groups[2]])
    assert seen == list(bb.contents.seen[:groups[2]]) and used == list(bb.contents.used[:groups[2]])
    assert 0 < sum(used) < sum(seen) and sum(used) == trained, "the draw left no window out: the case shows nothing"
    lib.rnn_amd_balanced_free(ba)
    lib.rnn_amd_balanced_free(bb)
    ga.close()
    gb.close()


def test_a_noisy_net_takes_the_per_generation_route(amd):
    lib, groups, n, T = amd, cc.GAP, 5, 4
    ga, gb = twins(lib, set_kw(n, 24, 3, groups, noise=0.1))
    x, tg = cc.block_of(T, n, N_IN, groups, 84, silent=(1,))
    train_windows(lib, ga, x, tg, groups[0], groups[1])
    cc.run_loop(lib, gb, x, tg, groups)
    snap = hold_twins(ga, gb, "presynaptic noise")
    fresh = sc.AmdBatchedSet(lib, **set_kw(n, 24, 3, groups, noise=0.1))
    assert not np.array_equal(snap["rng"], fresh.snapshot()["rng"]), "no noise was drawn"
    for gs in (ga, gb, fresh):
        gs.close()


# ------------------------------------------------------------------ 2. the gate script --

def write_gate_net(lib, gs, c):
    n0, b0 = gs.net.contents, gs.net.contents.bptt.contents
    lib.rnn_amd_sync_host(gs.net, rc.RNN_AMD_EVERYTHING)
    ih_w, ho_w, ih_m, ho_m = cc.gate_net(rc.view(n0.ih_weights, gs.I, gs.H), rc.view(n0.ho_weights, gs.H, gs.O), c)
    for ptr, a, shape in ((n0.ih_weights, ih_w, (gs.I, gs.H)), (n0.ho_weights, ho_w, (gs.H, gs.O)),
                          (b0.ih_momentum, ih_m, (gs.I, gs.H)), (b0.ho_momentum, ho_m, (gs.H, gs.O))):
        rc.view(ptr, *shape)[:] = a
    lib.rnn_amd_host_written(gs.net, rc.RNN_AMD_WEIGHTS | rc.RNN_AMD_MOMENTUMS)
    gs.stats(clear=True)


@pytest.mark.parametrize("c", [cc.GATE, cc.GATE_LARGE], ids=["small", "512 hidden, 128 channels: planes"])
def test_the_gate_script(amd, harness, c):
    lib, groups = amd, cc.ONE_OF_2
    kw = cc.gate_kw(c)
    if c is cc.GATE_LARGE:
        # the delta call of this shape leaves its sums as planes, which k_apply adds up under a closed gate
        o = sc.OracleSet(**kw)
        p = calc.plan(harness, input=c["n_in"], hidden=c["hidden"], output=2, streams=c["n"], depth=c["D"], accumulate=0, defer=1,
                      fuse_want=0, active=1, dense_inputs=1, flags=calc.TOP_DONE, own_slab_floats=8 * o.I * o.H + 64 * 128 * o.H)
        o.close()
        assert not p["small"] and not p["direct_fuse"], "the delta call of this shape leaves no planes"
    whole, single, loop = (sc.AmdBatchedSet(lib, **kw) for _ in range(3))
    for gs in (whole, single, loop):
        write_gate_net(lib, gs, c)
    x, tg = cc.gate_block(c)
    T = len(cc.GATE_SCRIPT)
    o = sc.OracleSet(**kw)
    start = single.snapshot()
    _sync_oracle_to(o, start)
    assert np.abs(start["ih_m"]).max() > 0 and np.abs(start["ho_m"]).max() > 0
    train_windows(lib, whole, x, tg, groups[0], groups[1])
    cc.run_loop(lib, loop, x, tg, groups)
    if c is cc.GATE_LARGE:      # the loop's last, closed generation left planes nobody has added up yet
        assert lib.rnn_amd_set_deferred(loop.handle) & rc.DEFERRED_IH_PLANES
    updates, before = [], start
    for t in range(T):
        train_windows(lib, single, x[t:t + 1], tg[t:t + 1], groups[0], groups[1])
        now = single.snapshot()
        trained, wrong, each, updated, wins = cc.oracle_generation(o, x[t], tg[t], groups, flags=FLAGS)
        so = o.snapshot()
        updates.append(updated)
        print("generation %d (%s): trained %d, wrongness %.9g, update %d" % (t, cc.GATE_SCRIPT[t], trained, wrong, updated))
        moved = not all(same(now[k], before[k]) for k in ("ih_w", "ho_w", "ih_m", "ho_m"))
        assert moved == cc.GATE_WANT[t], "generation %d (%s)" % (t, cc.GATE_SCRIPT[t])
        _same_mask(now["hidden"], so["hidden"])
        keys = ["ih_w", "ho_w", "ih_m", "ho_m", "hidden", "output", "hist"]
        if updated:
            keys += ["ih_delta", "ho_delta", "o_error"]
        replay.check(now, so, RTOL, keys=keys, exact=("index", "generation"))
        before = now
    assert tuple(updates) == cc.GATE_WANT
    o.close()
    hold_twins(whole, single, "one block against five")
    final = hold_twins(whole, loop, "the block against the loop")      # (the delta arrays after a closed generation among them)
    assert final["generation"][0] == sum(1 for k in cc.GATE_SCRIPT if k != "unlabelled")
    for gs in (whole, single, loop):
        gs.close()


# ------------------------------------------------------------------ 3. against the oracle twin --

@pytest.mark.parametrize("case", cc.PARITY_CASES, ids=lambda c: c[0])
def test_one_block_from_the_devices_state(amd, case):
    lib = amd
    name, hidden, n, D, groups, seed = case
    kw = cc.parity_kw(case)
    gs = sc.AmdBatchedSet(lib, **kw)
    warm = cc.block_of(D + 1, n, cc.PARITY_N_IN, groups, [seed, 99])
    train_windows(lib, gs, warm[0], warm[1], groups[0], groups[1])      # the ring is warmed on the device
    o = sc.OracleSet(**kw)
    for attempt in range(4):
        # (a hidden pre-activation within rounding of zero may land on either side in another summation order: such a
        # block is not a parity case -- tests/test_gpu_callers.py)
        _sync_oracle_to(o, gs.snapshot())
        x, tg = cc.parity_block(case, attempt)
        gs.stats(clear=True)
        trained = train_windows(lib, gs, x, tg, groups[0], groups[1])
        wrong, wins = 0.0, 0
        for t in range(x.shape[0]):
            r = cc.oracle_generation(o, x[t], tg[t], groups, flags=FLAGS)
            wrong, wins = wrong + r[1], wins + r[4]
        sg, so, st = gs.snapshot(), o.snapshot(), gs.stats()
        if np.array_equal(sg["hidden"] != 0, so["hidden"] != 0):
            break
        _same_mask(sg["hidden"], so["hidden"])
    else:
        raise AssertionError("no block without a rounding-level mask flip in 4 attempts")
    gs.close()
    o.close()
    replay.check(sg, so, RTOL, keys=["ih_delta", "ho_delta", "ih_w", "ho_w", "ih_m", "ho_m", "hidden", "output", "hist",
                                     "o_error", "min_error_factor", "ih_scale"], exact=("index", "generation"))
    print("%s: error %.9g, the oracle's %.9g, count %d, correct %d" % (name, st.error, wrong, st.count, st.correct))
    assert (st.count, st.correct) == (trained, wins) and abs(st.error - wrong) <= RTOL * wrong


# ------------------------------------------------------------------ 4. what the call leaves --

def test_a_net_outside_the_set_is_left_alone_and_the_deferred_state_is_the_loops(amd):
    lib, groups, n, T = amd, cc.GAP, 7, 3
    other = sc.AmdBatchedSet(lib, **set_kw(3, 24, 2, groups, seed=5))
    ox, otg = cc.block_of(1, 3, N_IN, groups, 85)
    cc.run_loop(lib, other, ox, otg, groups)      # (it has device state of its own)
    was = other.snapshot()
    ga, gb = twins(lib, set_kw(n, 99, 4, groups))
    x, tg = cc.block_of(T, n, N_IN, groups, 86)
    train_windows(lib, ga, x, tg, groups[0], groups[1])
    cc.run_loop(lib, gb, x, tg, groups)
    da, db = lib.rnn_amd_set_deferred(ga.handle), lib.rnn_amd_set_deferred(gb.handle)
    assert da == db, "the call leaves other deferred state than the loop: 0x%x, 0x%x" % (da, db)
    hold_twins(ga, gb, "after the deferred state was read")
    now = other.snapshot()
    for k in was:
        assert np.array_equal(was[k], now[k]) if was[k].dtype.kind != "f" else same(was[k], now[k]), "the other net's %s" % k
    for gs in (ga, gb, other):
        gs.close()


# ------------------------------------------------------------------ 5. the tool --

def test_the_tool_writes_the_same_net_whatever_the_block(amd, tmp_path):
    exe = os.path.join(rc.ROOT, "build", "classify_train_amd")
    nets = []
    for block in (1, 16):
        path = str(tmp_path / ("block%d.net" % block))
        r = subprocess.run([exe, "-H", "64", "-c", "8", "-d", "4", "-g", "40", "-r", "20", "-b", "1.5", "-B", str(block), "-o", path],
                           capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-3000:] + r.stdout[-1000:]
        assert "saved, loaded, metadata and sizes agree" in r.stdout
        with open(path, "rb") as f:
            nets.append(f.read())
    assert len(nets[0]) > 1000 and nets[0] == nets[1]


# ------------------------------------------------------------------ 6. the shared block buffer --

def test_the_block_trainers_share_one_buffer(amd):
    """One engine (hidden 24, 4 streams, depth 3) takes a parrot block of 2 steps (rnn_amd_set_dense_steps_tanh), then a
    block of 3 windows that is larger, so that the engine's one block buffer grows under it, then the parrot block again,
    which finds the grown buffer holding the windows.  Each call's result equals the same call made on a fresh engine whose
    buffer it is the first to touch -- brought to the same state by the per-generation loops, which the tests above and
    test_gpu_parrot_training.py hold to the blocks bit for bit and which use no block buffer -- in every array of the
    snapshot (weights, momentums, deltas, ...) and in the statistics."""
    lib, groups, n = amd, cc.GAP, 4
    kw = set_kw(n, 24, 3, groups)
    frames = np.ascontiguousarray(np.random.default_rng(91).uniform(-1, 1, (3, n, N_IN)).astype(F))
    x, tg = cc.block_of(3, n, N_IN, groups, 92)
    assert frames.nbytes < x.nbytes + tg.nbytes, "the block of windows is the larger one"
    width = groups[2]

    def parrot_loop(gs):
        for t in range(len(frames) - 1):
            a, b = np.ascontiguousarray(frames[t]), np.ascontiguousarray(frames[t + 1])
            lib.rnn_amd_set_dense_step_tanh(gs.handle, rc.fptr(a), a.shape[1], rc.fptr(b), b.shape[1], width, rc.WEIGHTED, 0.95)

    shared, fresh1, fresh2, fresh3 = twins(lib, kw, 4)
    train_frames(lib, shared, frames, width)
    train_frames(lib, fresh1, frames, width)
    hold_twins(shared, fresh1, "parrot's block, the buffer's first use")
    train_windows(lib, shared, x, tg, groups[0], groups[1])
    parrot_loop(fresh2)
    train_windows(lib, fresh2, x, tg, groups[0], groups[1])
    hold_twins(shared, fresh2, "the windows, in the buffer they grew")
    train_frames(lib, shared, frames, width)
    parrot_loop(fresh3)
    cc.run_loop(lib, fresh3, x, tg, groups)
    train_frames(lib, fresh3, frames, width)
    snap = hold_twins(shared, fresh3, "parrot's block again, in the windows' buffer")
    assert shared.stats().count > 0 and np.abs(snap["ih_delta"]).max() > 0
    for gs in (shared, fresh1, fresh2, fresh3):
        gs.close()

