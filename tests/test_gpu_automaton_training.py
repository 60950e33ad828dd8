"""Rnnca's trainer on the device (gstrnnca.c: fill_net_inputs 669-691, train_net 693-716, maybe_learn 718-750):
rnn_amd_set_automaton_steps (k_automaton_train_rows, the sigmoid loss with its statistics) and tools/rnnca_train_amd.

  1. the block is the loop, bit for bit: one call against rnn_amd_set_dense_step_sigmoid_mse (behind rnn_amd_set_advance
     where `advance`) on rows gathered by the numpy restatement (tests/automaton_train_cases.py), twin sets held equal in
     every array and generator;
  2. three generations from the device's state against the oracle twin at the project's parity bar;
  3. the statistics against the float64 sum over the restated answers, in the one-launch form and in the separate one, and
     the three existing sigmoid calls leaving them alone;
  4. a saturated written net on films of all 0 and all 255, and the sigmoid loss's non-finite rule on one planted row;
  5. a net outside the set is left alone and the deferred state after the call is the loop's;
  6. tools/rnnca_train_amd learns the CPU half's designed film and tools/rnnca_play_amd plays the saved net.
tests/test_automaton_train_cases_cpu.py shows on the oracle alone that these cases can notice a failure."""
import os
import subprocess

import numpy as np
import pytest

import automaton_train_cases as ac
import recur_ctypes as rc
import replay
import scenarios as sc
from recur_amd.drivers import train_automaton
from test_gpu_callers import _same_mask, _sync_oracle_to

pytestmark = pytest.mark.gpu
F = np.float32
RTOL = ac.PARITY_BAR
M = ac.MOMENTUM


@pytest.fixture(scope="module")
def amd():
    lib = rc.load_amd()
    assert lib.rnn_amd_device_count() >= 1, "no HIP device: the product has no CPU fallback"
    rc.bind_char(lib)
    return lib


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


def hold_twins(ga, gb, what):
    """every array of the two sets' snapshots equal bit for bit: weights, momentums, deltas, hidden rows, rings, outputs,
    error rows, ring indices, generations and generators"""
    sa, sb = ga.snapshot(), gb.snapshot()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]) if sa[k].dtype.kind != "f" else same(sa[k], sb[k]), "%s: %s differs" % (what, k)
    return sa


def set_kw(g, n, hidden, D, n_out=3, noise=0.0, **more):
    kw = dict(input_size=g.input_size, hidden_size=hidden, output_size=n_out, S=n, D=D, seed=61, momentum=M, noise=noise,
              learn_rate=1e-5 if hidden > 1000 else 1e-3)
    kw.update(more)
    return kw


def block_data(g, T, n, seed, moving=False):
    xy = ac.random_xy(g, n, seed, T=T if moving else None)
    return ac.plant(g, ac.film_of(g, T, seed), xy), xy


# ------------------------------------------------------------------ 1. the block is the loop --

G54, G54W, G33, G33W = ac.Grid(5, 4), ac.Grid(5, 4, edges=0), ac.Grid(3, 3), ac.Grid(3, 3, edges=0)
# (name, grid, T, trainers, hidden, depth, outputs, noise, advance, positions per step)
BLOCKS = (
    [("T %d, %d trainers" % (T, n), (G54, G54W, G33, G33W)[k % 4], T, n, 99, (1, 10)[k % 2], 3, 0.0, k % 3 == 0, k % 2 == 1)
     for T in (1, 5) for k, n in enumerate((1, 3, 4, 63, 64, 65, 200, 257))] +
    [("hidden 512", G54, 5, 65, 512, 10, 3, 0.0, True, True),
     ("hidden 512, depth 1, no advance", G33W, 5, 9, 512, 1, 3, 0.0, False, False),
     ("hidden 1024", G54W, 1, 64, 1024, 10, 3, 0.0, True, False),
     ("8 outputs", G54, 5, 7, 99, 10, 8, 0.0, True, True),
     ("70 outputs: the separate loss kernel", G54, 5, 7, 99, 10, 70, 0.0, True, True),
     ("presynaptic noise", G54W, 5, 65, 99, 10, 3, 0.1, True, True),
     ("presynaptic noise, no advance", G54, 5, 4, 99, 1, 3, 0.1, False, False),
     ("len_pos 3", ac.Grid(5, 4, len_pos=3), 5, 7, 99, 10, 3, 0.0, False, True),
     ("144 x 96", ac.Grid(144, 96), 2, 200, 99, 10, 3, 0.0, False, True)])


@pytest.mark.parametrize("c", BLOCKS, ids=lambda c: c[0])
def test_the_block_is_the_loop_bit_for_bit(amd, c):
    lib = amd
    name, g, T, n, hidden, D, n_out, noise, advance, moving = c
    kw = set_kw(g, n, hidden, D, n_out, noise)
    ga, gb = sc.AmdBatchedSet(lib, **kw), sc.AmdBatchedSet(lib, **kw)
    film, xy = block_data(g, T, n, [T, n, hidden], moving)
    planted = None
    if n_out > 3:      # an error row planted behind the three scored columns: it stays what it was
        planted = np.zeros((n, ga.O), F)
        planted[:, 3:n_out] = np.random.default_rng(2).uniform(0.05, 0.2, (n, n_out - 3)).astype(F)
        for gs in (ga, gb):
            lib.rnn_amd_set_put_o_error(gs.handle, rc.fptr(planted), gs.O)
    assert train_automaton(lib, ga, g.geometry(), film, xy, advance=advance, momentum=M) == T
    ac.run_loop(lib, gb, g, film, xy, advance=advance)
    snap = hold_twins(ga, gb, name)
    assert int(snap["generation"][0]) == T
    assert np.abs(snap["o_error"][:, :3]).max() > 0 and (snap["output"][:, :3] > 0).all() and (snap["output"][:, :3] < 1).all()
    if planted is not None:
        assert same(snap["o_error"][:, 3:], planted[:, 3:]), "error columns from 3 on were touched"
        assert (np.abs(snap["output"][:, 3:n_out]) > 0).any()      # (raw outputs, the twin's: held above)
    ga.close()
    gb.close()


def test_fixed_positions_are_the_same_positions_repeated(amd):
    lib, g, T, n = amd, G54, 5, 7
    kw = set_kw(g, n, 99, 10)
    ga, gb = sc.AmdBatchedSet(lib, **kw), sc.AmdBatchedSet(lib, **kw)
    film, xy = block_data(g, T, n, 5)
    train_automaton(lib, ga, g.geometry(), film, xy, momentum=M)
    train_automaton(lib, gb, g.geometry(), film, ac.per_step(xy, T), momentum=M)
    hold_twins(ga, gb, "fixed against repeated")
    ga.close()
    gb.close()


@pytest.mark.parametrize("advance", [False, True])
def test_blocks_chain_on_their_shared_frame(amd, advance):
    lib, g, n = amd, G54W, 7
    kw = set_kw(g, n, 99, 4)
    ga, gb = sc.AmdBatchedSet(lib, **kw), sc.AmdBatchedSet(lib, **kw)
    film, xy = block_data(g, 5, n, 6, moving=True)
    ga.stats(clear=True), gb.stats(clear=True)
    train_automaton(lib, ga, g.geometry(), film, xy, advance=advance, momentum=M)
    train_automaton(lib, gb, g.geometry(), film[:3], xy[:2], advance=advance, momentum=M)
    train_automaton(lib, gb, g.geometry(), film[2:], xy[2:], advance=advance, momentum=M)
    hold_twins(ga, gb, "2 + 3")
    ta, tb = ga.stats(), gb.stats()
    assert (ta.count, ta.error) == (tb.count, tb.error) and ta.count == 5 * n
    ga.close()
    gb.close()


def test_conditioning_is_rnn_condition_net_in_the_loop(amd):
    """the net's conditioning flags on (scale and zero), nine generations from generation 0: the scale interval
    (generation % 8 == 0) and the zero interval (== 2) are both crossed"""
    lib, g, n, T = amd, G54, 7, 9
    flags = rc.FLAG_STANDARD | rc.FLAG_ADAPTIVE_MIN_ERROR | rc.COND_USE_SCALE | rc.COND_USE_ZERO
    kw = set_kw(g, n, 64, 4, flags=flags)
    ga, gb, gc = (sc.AmdBatchedSet(lib, **kw) for _ in range(3))
    film, xy = block_data(g, T, n, 7, moving=True)
    train_automaton(lib, ga, g.geometry(), film, xy, advance=True, momentum=M, condition=True)
    ac.run_loop(lib, gb, g, film, xy, advance=True, condition=True)
    ac.run_loop(lib, gc, g, film, xy, advance=True, condition=False)
    hold_twins(ga, gb, "conditioned")
    assert int(ga.snapshot()["generation"][0]) == T
    assert not same(ga.snapshot()["ih_w"], gc.snapshot()["ih_w"]), "the conditioning left no trace: the case shows nothing"
    for gs in (ga, gb, gc):
        gs.close()


def test_a_soft_start_is_the_loop_handed_the_restated_momenta(amd):
    lib, g, n, T, soft = amd, G54, 7, 5, 3.0
    kw = set_kw(g, n, 99, 4)
    ga, gb, gc = (sc.AmdBatchedSet(lib, **kw) for _ in range(3))
    film, xy = block_data(g, T, n, 8, moving=True)
    momenta = ac.np_momenta(0, T, 0.95, soft)
    assert len(set(float(m) for m in momenta)) == T and max(momenta) < 0.95      # every generation its own, none the cap
    train_automaton(lib, ga, g.geometry(), film, xy, momentum=0.95, soft_start=soft)
    ac.run_loop(lib, gb, g, film, xy, momenta=momenta)
    ac.run_loop(lib, gc, g, film, xy, momentum=0.95)
    hold_twins(ga, gb, "soft start")
    assert not same(ga.snapshot()["ih_w"], gc.snapshot()["ih_w"]), "the soft start left no trace"
    # chained, the second block reads the net's generation where the first left it
    train_automaton(lib, ga, g.geometry(), film[:3], xy[:2], momentum=0.95, soft_start=soft)
    ac.run_loop(lib, gb, g, film[:3], xy[:2], momenta=ac.np_momenta(T, 2, 0.95, soft))
    hold_twins(ga, gb, "soft start, the second block")
    for gs in (ga, gb, gc):
        gs.close()


# ------------------------------------------------------------------ 2. against the oracle twin --

@pytest.mark.parametrize("activation,advance", [(rc.RELU, False), (rc.RELU, True), (rc.RESQRT, True), (rc.RECLIP20, False)])
def test_three_generations_from_the_devices_state(amd, activation, advance):
    lib, g, n, D, T = amd, G54, 20, 4, 3
    kw = set_kw(g, n, 64, D, activation=activation)
    gs = sc.AmdBatchedSet(lib, **kw)
    film, xy = block_data(g, D + 2, n, 9, moving=True)
    train_automaton(lib, gs, g.geometry(), film, xy, advance=advance, momentum=M)      # the ring is warmed on the device
    o = sc.OracleSet(**kw)
    for attempt in range(4):
        # (a hidden pre-activation within rounding of zero may land on either side in another summation order: such a
        # block is not a parity case -- tests/test_gpu_callers.py, _rnnca_generation)
        _sync_oracle_to(o, gs.snapshot())
        film, xy = block_data(g, T, n, [10, attempt], moving=True)
        gs.stats(clear=True)
        train_automaton(lib, gs, g.geometry(), film, xy, advance=advance, momentum=M)
        rows, targets = ac.np_block(g, film, xy)
        terms = [ac.oracle_generation(o, rows[t], targets[t], M, advance) for t in range(T)]
        sg, so, st = gs.snapshot(), o.snapshot(), gs.stats()
        if np.array_equal(sg["hidden"] != 0, so["hidden"] != 0):
            break
        _same_mask(sg["hidden"], so["hidden"])
    else:
        raise AssertionError("no block without a rounding-level mask flip in 4 attempts")
    gs.close()
    o.close()
    assert np.abs(so["o_error"][:, :3]).max() > 0 and (so["o_error"][:, 3:] == 0).all()
    replay.check(sg, so, RTOL, keys=["ih_delta", "ho_delta", "ih_w", "ho_w", "ih_m", "ho_m", "hidden", "output", "hist",
                                     "o_error", "min_error_factor", "ih_scale"], exact=("index", "generation"))
    want = float(np.stack(terms).astype(np.float64).sum())
    print("error %.9g, the oracle's terms %.9g, count %d" % (st.error, want, st.count))
    assert st.count == T * n and abs(st.error - want) <= RTOL * want, (st.count, st.error, want)


# ------------------------------------------------------------------ 3. the statistics --

def loop_with_terms(lib, gs, g, film, xy, advance):
    """the loop, generation by generation, and the float64 sum of (target - a)^2 over the answers it leaves"""
    rows, targets = ac.np_block(g, film, xy)
    total = 0.0
    for t in range(rows.shape[0]):
        ac.run_loop(lib, gs, g, film[t:t + 2], ac.per_step(xy, rows.shape[0])[t:t + 1], advance=advance)
        a = gs.snapshot()["output"][:, :3].astype(np.float64)
        total += float(((targets[t].astype(np.float64) - a) ** 2).sum())
    return total


@pytest.mark.parametrize("form,n_out,noise", [("one launch", 3, 0.0), ("separate: 70 outputs", 70, 0.0),
                                              ("separate: presynaptic noise", 3, 0.1)])
def test_error_and_count(amd, form, n_out, noise):
    lib, g, n, T = amd, G54, 65, 5
    kw = set_kw(g, n, 99, 4, n_out, noise)
    ga, gb = sc.AmdBatchedSet(lib, **kw), sc.AmdBatchedSet(lib, **kw)
    film, xy = block_data(g, T, n, 11, moving=True)
    ga.stats(clear=True), gb.stats(clear=True)
    train_automaton(lib, ga, g.geometry(), film, xy, advance=True, momentum=M)
    want = loop_with_terms(lib, gb, g, film, xy, True)
    hold_twins(ga, gb, form)
    sa, sb = ga.stats(), gb.stats()
    print("%s: error %.9g, the float64 restatement %.9g, count %d" % (form, sa.error, want, sa.count))
    assert sa.count == T * n
    assert want > 0 and abs(sa.error - want) <= 1e-4 * want, (sa.error, want)
    assert (sb.count, sb.error) == (0, 0.0), "the loop's calls touched the statistics"
    ga.close()
    gb.close()


def test_the_existing_sigmoid_calls_leave_the_statistics_alone(amd):
    lib, g, n = amd, G54, 7
    for n_out in (3, 70):      # the one-launch top, and past it
        gs = sc.AmdBatchedSet(lib, **set_kw(g, n, 99, 4, n_out))
        film, xy = block_data(g, 2, n, 12)
        gs.stats(clear=True)
        train_automaton(lib, gs, g.geometry(), film, xy, momentum=M)
        before = gs.stats()
        assert before.count == 2 * n and before.error > 0
        rows, targets = ac.np_block(g, film, xy)
        x, t = np.ascontiguousarray(rows[0]), np.ascontiguousarray(targets[0])
        lib.rnn_amd_set_opinion(gs.handle, rc.fptr(x), x.shape[1], None)
        lib.rnn_amd_set_sigmoid_mse_error(gs.handle, rc.fptr(t), 3, 3)
        lib.rnn_amd_set_opinion_sigmoid_mse(gs.handle, rc.fptr(x), x.shape[1], rc.fptr(t), 3, 3)
        lib.rnn_amd_set_dense_step_sigmoid_mse(gs.handle, rc.fptr(x), x.shape[1], rc.fptr(t), 3, 3, rc.WEIGHTED, M)
        after = gs.stats()
        for field in ("error", "count", "entropy", "correct"):
            a, b = getattr(before, field), getattr(after, field)
            assert np.array([a]).tobytes() == np.array([b]).tobytes(), (n_out, field, a, b)
        gs.close()


# ------------------------------------------------------------------ 4. extremes --

def write_net(lib, gs, ih, ho):
    lib.rnn_amd_sync_host(gs.net, rc.RNN_AMD_EVERYTHING)
    rc.view(gs.net.contents.ih_weights, gs.I, gs.H)[:] = ih
    rc.view(gs.net.contents.ho_weights, gs.H, gs.O)[:] = ho
    lib.rnn_amd_host_written(gs.net, rc.RNN_AMD_WEIGHTS)


@pytest.mark.parametrize("level", [0, 255])
def test_saturated_net_on_a_flat_film(amd, level):
    """the top layer is its bias row alone, +-100: fast_sigmoid answers exactly 1 and 0, so the slope a (1 - a) and the
    error are exactly 0 against any target, and so is every delta"""
    lib, g, n, T = amd, G54, 7, 3
    gs = sc.AmdBatchedSet(lib, **set_kw(g, n, 24, 3))
    ho = np.zeros((gs.H, gs.O), F)
    ho[0, :3] = [100.0, -100.0, 100.0]
    write_net(lib, gs, np.zeros((gs.I, gs.H), F), ho)
    film = np.full((T + 1, 3, g.height, g.width), level, np.uint8)
    gs.stats(clear=True)
    train_automaton(lib, gs, g.geometry(), film, ac.random_xy(g, n, 13), advance=True, momentum=M)
    snap, st = gs.snapshot(), gs.stats()
    gs.close()
    assert same(snap["output"][:, :3], np.tile(np.array([1.0, 0.0, 1.0], F), (n, 1)))
    for k in ("o_error", "ho_delta", "ih_delta"):
        assert (snap[k] == 0).all(), k          # (zeros of either sign: the slope 0 times a difference)
    target = float(ac.np_unit(level))
    want = n * T * sum((target - a) ** 2 for a in (1.0, 0.0, 1.0))
    assert st.count == n * T and abs(st.error - want) <= 1e-4 * max(want, 1e-30), (st.error, want)


def planted_run(lib, poison):
    """seven trainers on 5 x 4; the film is 0 but for luma 255 under trainer 2, whose first input -- its own cell's luma --
    is then exactly 1 and everyone else's 0.  That input lights hidden unit 1 alone (weight 2), and unit 1 feeds output 1
    with 2e38 (poison: 2 * 2e38 overflows to an infinity in trainer 2's row, an exact 0 in the others') or with 0.125 (the
    control).  The bias row gives every output a finite part."""
    g, n = G54, 7
    gs = sc.AmdBatchedSet(lib, **set_kw(g, n, 24, 3, learn_rate=0.0))
    xy = np.array([(0, 0), (4, 3), (2, 1), (4, 0), (0, 3), (3, 3), (1, 2)], np.int32)
    film = np.zeros((2, 3, g.height, g.width), np.uint8)
    film[:, 0, 1, 2] = 255
    ih, ho = np.zeros((gs.I, gs.H), F), np.zeros((gs.H, gs.O), F)
    ih[1 + 24 + 0, 1] = 2.0
    ho[0, :3] = [0.5, -1.0, 2.0]
    ho[1, 1] = 2e38 if poison else 0.125
    write_net(lib, gs, ih, ho)
    gs.stats(clear=True)
    train_automaton(lib, gs, g.geometry(), film, xy, advance=True, momentum=M)
    snap, st = gs.snapshot(), gs.stats()
    train_automaton(lib, gs, g.geometry(), film, xy, advance=True, momentum=M)      # (every call returns)
    gs.close()
    return snap, st


def test_the_non_finite_rule_on_one_planted_row(amd):
    """the sigmoid loss's rule (include/recur_amd.h, "OUTPUTS THAT ARE NOT FINITE"): the sigmoid of an output that is not
    finite is NaN and so is its error, elementwise; every other output of that row and every other row is the control's bit
    for bit, and every call returns"""
    p, ps = planted_run(amd, True)
    c, cs = planted_run(amd, False)
    bad = np.zeros((7, 3), bool)
    bad[2, 1] = True
    assert np.isfinite(c["output"][:, :3]).all() and np.isfinite(c["o_error"][:, :3]).all() and np.isfinite(cs.error)
    assert c["hidden"][2, 1] == 2.0 and (np.delete(c["hidden"][:, 1], 2) == 0).all()
    for k in ("output", "o_error"):
        assert np.array_equal(np.isnan(p[k][:, :3]), bad), k
        assert same(p[k][:, :3][~bad], c[k][:, :3][~bad]), k
    assert same(p["hidden"], c["hidden"])
    assert ps.count == cs.count == 7 and np.isnan(ps.error)


# ------------------------------------------------------------------ 5. what the call leaves --

def test_a_net_outside_the_set_is_left_alone_and_the_deferred_state_is_the_loops(amd):
    lib, g, n, T = amd, G54, 7, 3
    kw = set_kw(g, n, 99, 4)
    other = sc.AmdBatchedSet(lib, **set_kw(g, 3, 24, 2, seed=5))
    film, xy = block_data(g, T, n, 14, moving=True)
    ac.run_loop(lib, other, g, film[:2], ac.random_xy(g, 3, 1))      # (it has device state of its own)
    was = other.snapshot()
    ga, gb = sc.AmdBatchedSet(lib, **kw), sc.AmdBatchedSet(lib, **kw)
    train_automaton(lib, ga, g.geometry(), film, xy, momentum=M)
    ac.run_loop(lib, gb, g, film, xy)
    da, db = lib.rnn_amd_set_deferred(ga.handle), lib.rnn_amd_set_deferred(gb.handle)
    assert da == db, "the call leaves other deferred state than the loop: 0x%x, 0x%x" % (da, db)
    hold_twins(ga, gb, "after the deferred state was read")
    now = other.snapshot()
    for k in was:
        assert np.array_equal(was[k], now[k]) if was[k].dtype.kind != "f" else same(was[k], now[k]), "the other net's %s" % k
    for gs in (ga, gb, other):
        gs.close()


# ------------------------------------------------------------------ 6. learning, through the tool --

def test_the_tool_learns_and_the_player_plays_its_net(amd, tmp_path):
    L = ac.LEARN
    build = os.path.join(rc.ROOT, "build")
    film, netfile, played = str(tmp_path / "film.u8"), str(tmp_path / "rnnca.net"), str(tmp_path / "played.u8")
    ac.learning_film().tofile(film)
    r = subprocess.run([os.path.join(build, "rnnca_train_amd"), "-w", str(L["width"]), "-h", str(L["height"]), "-p", L["pattern"],
                        "-t", str(L["trainers"]), "-H", str(L["hidden"]), "-d", str(L["depth"]), "-r", str(L["rate"]), "-m",
                        str(L["momentum"]), "-b", str(L["block"]), "-s", str(L["seed"]), film, netfile],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln.split() for ln in r.stdout.strip().splitlines()]
    print(r.stdout)
    assert len(lines) == L["generations"] // L["block"] and int(lines[-1][0]) == L["generations"]
    first, last = float(lines[0][1]), float(lines[-1][1])
    assert np.isfinite(first) and np.isfinite(last) and last < ac.LEARN_FACTOR * first, (first, last)
    frames = 4
    r = subprocess.run([os.path.join(build, "rnnca_play_amd"), "-w", str(L["width"]), "-h", str(L["height"]), "-p", L["pattern"],
                        "-n", str(frames), "-i", film, netfile, played], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.fromfile(played, np.uint8)
    assert got.size == frames * 3 * L["width"] * L["height"] and len(np.unique(got)) > 4
