"""That the GPU cases of tests/test_gpu_automaton_training.py can notice a failure, shown on the oracle alone (orc_opinion,
orc_sigmoid_mse_error, orc_calc_deltas, orc_apply_learning, orc_advance) without a device: each thing the block call could
get wrong -- a trainer one pixel off, the ring advanced or not, the soft start, the positions of a later generation --
moves the weights after the case's generations beyond the parity bar the device is held to.  And the film of the tool test
is one the oracle learns: its mean squared error falls to less than LEARN_FACTOR / 2 of what it was, so that the tool's
bar of LEARN_FACTOR has a margin of two."""
import numpy as np

import automaton_train_cases as ac
import recur_ctypes as rc
import scenarios as sc

F = np.float32
BEYOND = 10 * ac.PARITY_BAR      # ten times the bar: a failure of this kind cannot hide under it


def weights_after(film, xy, advance=False, soft_start=0.0, momentum=ac.MOMENTUM):
    c = ac.SENS
    o = sc.OracleSet(**ac.sens_kw(c))
    ac.oracle_block(o, c["grid"], film, xy, advance=advance, momentum=momentum, soft_start=soft_start)
    snap = o.snapshot()
    o.close()
    return snap


def moved(a, b):
    return max(rc.rel_err(a[k], b[k]) for k in ("ih_w", "ho_w"))


def test_a_trainer_one_pixel_off_is_noticed():
    film, xy = ac.sens_data()
    base = weights_after(film, xy)
    for axis in (0, 1):
        off = xy.copy()
        j = int(np.argmax(off[0, :, axis] < (ac.SENS["grid"].width, ac.SENS["grid"].height)[axis] - 1))
        off[:, j, axis] += 1
        assert off[:, :, 0].max() < ac.SENS["grid"].width and off[:, :, 1].max() < ac.SENS["grid"].height
        e = moved(weights_after(film, off), base)
        print("trainer %d moved along axis %d: weights differ by %.3g" % (j, axis, e))
        assert e > BEYOND


def test_advance_0_against_1_is_noticed():
    film, xy = ac.sens_data()
    e = moved(weights_after(film, xy, advance=True), weights_after(film, xy, advance=False))
    print("advance: weights differ by %.3g" % e)
    assert e > BEYOND


def test_a_soft_start_is_noticed():
    film, xy = ac.sens_data()
    e = moved(weights_after(film, xy, soft_start=3.0, momentum=0.95), weights_after(film, xy, momentum=0.95))
    print("soft start: weights differ by %.3g" % e)
    assert e > BEYOND


def test_positions_per_step_against_fixed_are_noticed():
    film, xy = ac.sens_data()
    assert not np.array_equal(xy[0], xy[-1])
    e = moved(weights_after(film, xy), weights_after(film, xy[0]))
    print("positions per step: weights differ by %.3g" % e)
    assert e > BEYOND


def learning_positions(generations):
    """trainers inside a margin of 2, one of them moved after every 8th generation, as the tool places them (from another
    generator: the film's rule holds at every cell inside the margin)"""
    L = ac.LEARN
    rs = np.random.default_rng(L["seed"])
    cells = [(x, y) for y in range(2, L["height"] - 2) for x in range(2, L["width"] - 2)]
    now = [cells[i] for i in rs.permutation(len(cells))[:L["trainers"]]]
    out = np.zeros((generations, L["trainers"], 2), np.int32)
    for t in range(generations):
        out[t] = now
        if (t + 1) % 8 == 0:
            free = [c for c in cells if c not in now]
            now[int(rs.integers(len(now)))] = free[int(rs.integers(len(free)))]
    return out


def test_the_oracle_learns_the_designed_film():
    L = ac.LEARN
    g = ac.learning_grid()
    film = ac.learning_film()
    assert np.array_equal(film[1][:, :, 1:], film[0][:, :, :-1])      # every frame is the one before, one pixel on
    xy = learning_positions(L["generations"])
    o = sc.OracleSet(input_size=g.input_size, hidden_size=L["hidden"], output_size=3, S=L["trainers"], D=L["depth"],
                     learn_rate=L["rate"], seed=L["seed"], momentum=L["momentum"], flags=rc.FLAG_STANDARD)
    mse = ac.oracle_block(o, g, film, xy, advance=False, momentum=L["momentum"])
    o.close()
    first, last = float(np.mean(mse[:L["block"]])), float(np.mean(mse[-L["block"]:]))
    print("the oracle's mean squared error: first block %.6g, last block %.6g" % (first, last))
    assert last < 0.5 * ac.LEARN_FACTOR * first, (first, last)
