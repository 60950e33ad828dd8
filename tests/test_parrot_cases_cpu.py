"""The GPU cases of tests/test_gpu_parrot_training.py on the oracle alone: that they can notice a failure.  A raw answer
near the tanh's clamp at +-4.97 would make the comparison a matter of rounding, a saturated case that is not saturated
would hold nothing, planted error that is zero would hide a kernel that clears it, a learning signal that the oracle
cannot learn would say nothing about the device, and a generation whose advance, clear or channel sum can be dropped
without the snapshot moving would not test them."""
import numpy as np
import pytest

import parrot_cases as pc
import recur_ctypes as rc
import scenarios as sc

F = np.float32
RTOL = 1e-4   # the project's parity bar (tests/test_gpu_callers.py)


@pytest.mark.parametrize("c", pc.GENERATION_CASES, ids=lambda c: c["name"])
def test_raw_answers_stay_clear_of_the_clamp(c):
    """D + 3 free-running generations (the GPU test's warm-up and its compared generation): every raw answer inside
    |x| < 4, nowhere near +-4.97 where the bar's 1e-4 could move an answer across the clamp"""
    o, raws, _ = pc.free_running(c, c["D"] + 3)
    o.close()
    worst = max(float(np.abs(r).max()) for r in raws)
    assert np.isfinite(worst) and 0 < worst < 4.0, worst


def test_saturated_case_is_saturated():
    c = pc.SATURATED_CASE
    o, raws, losses = pc.free_running(c, c["D"] + 3)
    snap = o.snapshot()
    o.close()
    for r in raws:
        assert np.all(np.abs(r) > 4.97 * (1 + 1e-3))
    assert np.all(np.abs(snap["output"][:, :c["n"]]) == 1) and np.all(snap["o_error"] == 0)
    assert np.all(snap["ho_delta"] == 0) and np.all(snap["ih_delta"] == 0)


def test_planted_error_is_there():
    cases = [c for c in pc.GENERATION_CASES if c["n"] < c["n_out"]]
    assert cases
    for c in cases:
        _, _, planted = pc.case_data(c, 0)
        assert np.all(planted[:, c["n"]:] != 0)
        o, _, _ = pc.free_running(c, 1)
        kept = o.snapshot()["o_error"]
        o.close()
        assert np.array_equal(kept[:, c["n"]:c["n_out"]], planted[:, c["n"]:]) and np.all(kept[:, c["n_out"]:] == 0)


def learning_curve():
    L = pc.LEARN
    fr = pc.learning_frames()
    o = sc.OracleSet(input_size=256, hidden_size=L["hidden"], output_size=256, S=L["channels"], D=L["depth"],
                     learn_rate=L["rate"], seed=L["seed"], momentum=pc.MOMENTUM)
    means = []
    for t in range(L["generations"]):
        _, loss = pc.oracle_generation(o, fr[t], fr[t + 1], 256)
        means.append(float(loss.astype(np.float64).mean()))
    o.close()
    return np.array(means)


def test_the_learning_signal_is_learnt_by_the_oracle():
    """the designed signal (two channels of travelling sines, hidden 32, 400 generations): the oracle's mean parrot_loss
    over the last quarter of the generations is under half of the first quarter's.  The oracle's two figures:
    first quarter 0.3886, last quarter 0.02028."""
    m = learning_curve()
    q = len(m) // 4
    first, last = float(m[:q].mean()), float(m[-q:].mean())
    print("first quarter %.4g, last quarter %.4g" % (first, last))
    assert last < 0.5 * first, (first, last)


@pytest.mark.parametrize("drop", ["advance", "clear", "accumulate"])
def test_each_part_of_the_generation_shows(drop):
    """dropping the advance, dropping the clear, or accumulate = 0 per stream (the plugin's overwrite) moves the oracle's
    snapshot beyond the bar"""
    c = pc.GENERATION_CASES[1]
    gens = c["D"] + 3

    def run(**switch):
        o = sc.OracleSet(**pc.case_kw(c))
        for gen in range(gens):
            x, t, planted = pc.case_data(c, gen)
            pc.oracle_generation(o, x, t, c["n"], planted, **(switch if gen == gens - 1 else {}))
        s = o.snapshot()
        o.close()
        return s

    want, got = run(), run(**{drop: False})
    keys = {"advance": ["hist", "ih_delta"], "clear": ["ih_delta", "ho_delta"], "accumulate": ["ih_delta", "ho_delta"]}[drop]
    for k in keys:
        assert rc.rel_err(got[k], want[k]) > 10 * RTOL, (k, rc.rel_err(got[k], want[k]))
    if drop == "advance":
        assert not np.array_equal(got["index"], want["index"])
