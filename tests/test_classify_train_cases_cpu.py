"""What tests/test_gpu_classify_training.py rests on, shown from the oracle alone (tests/classify_train_cases.py):

  * on the written saturated net a label of class 0 has a wrongness of exactly 0.0f and a label of class 1 has not, and no
    softmax likelihood exceeds 1 -- the one way the device's gate (some trained stream's wrongness is not 0) could differ
    from the reference's float sum (classify_train_rule.h) does not occur on the cases used;
  * the script's gates are the intended sequence: open, closed, unlabelled, open, closed;
  * applying the update in a closed generation would change the weights: the exact gate is observable;
  * in the oracle-comparison cases no trained group has its two best likelihoods closer than the parity bar can move them:
    zero unclear winners, so `correct` is the same count on a device within the bar."""
import numpy as np
import pytest

import classify_train_cases as cc
import recur_ctypes as rc
import scenarios as sc

F = np.float32
FLAGS = rc.FLAG_STANDARD | rc.FLAG_ADAPTIVE_MIN_ERROR


def gate_oracle(c=cc.GATE):
    o = sc.OracleSet(**cc.gate_kw(c))
    a = o.arrays()
    ih_w, ho_w, ih_m, ho_m = cc.gate_net(a["ih_w"], a["ho_w"], c)
    for k, v in (("ih_w", ih_w), ("ho_w", ho_w), ("ih_m", ih_m), ("ho_m", ho_m)):
        a[k][:] = v
    return o


def run_script(gate="reference"):
    """-> per generation (updated, every channel's likelihoods [S][2], its wrongness [S], the weights behind it)"""
    o = gate_oracle()
    x, tg = cc.gate_block()
    out = []
    for t in range(len(cc.GATE_SCRIPT)):
        like = []
        trained, wrong, each, updated, wins = cc.oracle_generation(o, x[t], tg[t], cc.ONE_OF_2, flags=FLAGS, gate=gate,
                                                                   likelihoods=like)
        snap = o.snapshot()
        out.append(dict(updated=updated, like=np.array(like, F), each=each, trained=trained, wrong=wrong, wins=wins,
                        ih_w=snap["ih_w"], ho_w=snap["ho_w"], ih_m=snap["ih_m"], ho_m=snap["ho_m"], output=snap["output"]))
    o.close()
    return out, tg


@pytest.fixture(scope="module")
def script():
    return run_script()


def test_class_0_is_exactly_right_and_class_1_is_not(script):
    gens, tg = script
    for t, g in enumerate(gens):
        like = g["like"]
        gap = g["output"][:, 0] - g["output"][:, 1]
        assert (gap > 70).all() and (gap < 90).all(), "a logit gap of about 80"
        assert (like <= F(1.0)).all() and (like >= 0).all(), "a likelihood above 1"
        assert (like[:, 0] == F(1.0)).all(), "class 0 is not certain"
        wrong1 = F(1.0) - like[:, 1]
        assert (wrong1 != 0).all() and (F(1.0) - like[:, 0] == 0).all()
        assert not np.signbit(F(1.0) - like[:, 0]).any()      # (+0: the sum of such terms is +0)
    # the wrongness the oracle's loss itself reports, where it is exact: the closed generations' channels all report 0
    for t, kind in enumerate(cc.GATE_SCRIPT):
        if kind == "closed":
            labelled = tg[t, :, 0] == 0
            assert labelled.any() and (gens[t]["each"][labelled] == 0).all() and gens[t]["wrong"] == 0.0
            assert gens[t]["trained"] == labelled.sum() == gens[t]["wins"]
        elif kind == "open":
            assert gens[t]["wrong"] >= 1.0 and (tg[t, :, 0] == 1).any() and (tg[t, :, 0] == 0).any()


def test_the_scripts_gates_are_the_intended_sequence(script):
    gens, tg = script
    assert tuple(g["updated"] for g in gens) == cc.GATE_WANT
    assert [g["trained"] > 0 for g in gens] == [k != "unlabelled" for k in cc.GATE_SCRIPT]
    masks, active, gen = cc.np_decisions(tg, cc.ONE_OF_2[1])
    assert (active > 0).tolist() == [k != "unlabelled" for k in cc.GATE_SCRIPT]


def test_an_update_in_a_closed_generation_would_change_the_weights(script):
    """the same script with "update whenever a group trained" (exact_gate 0): the first closed generation moves the weights
    by the momentum arrays, which is what the exact gate must not do"""
    gens, _ = script
    always, _ = run_script(gate="always")
    first_closed = cc.GATE_SCRIPT.index("closed")
    for k in ("ih_w", "ho_w", "ih_m", "ho_m"):
        assert np.array_equal(gens[first_closed - 1][k], always[first_closed - 1][k]), k      # the same until then
        assert np.array_equal(gens[first_closed][k], gens[first_closed - 1][k]), k           # closed: nothing moves
        assert not np.array_equal(always[first_closed][k], gens[first_closed][k]), k          # ... and this would have
    assert always[first_closed]["updated"] and not gens[first_closed]["updated"]


@pytest.mark.parametrize("case", cc.PARITY_CASES, ids=lambda c: c[0])
def test_no_unclear_winner_in_the_oracle_comparison_cases(case):
    name, hidden, n, D, groups, seed = case
    o = sc.OracleSet(**cc.parity_kw(case))
    warm = cc.block_of(D + 1, n, cc.PARITY_N_IN, groups, [seed, 99])
    for t in range(warm[0].shape[0]):
        cc.oracle_generation(o, warm[0][t], warm[1][t], groups, flags=FLAGS)
    x, tg = cc.parity_block(case, 0)
    unclear = trained = 0
    for t in range(x.shape[0]):
        like = []
        trained += cc.oracle_generation(o, x[t], tg[t], groups, flags=FLAGS, likelihoods=like)[0]
        like = np.array(like, F)
        assert (like <= F(1.0)).all(), "a likelihood above 1"
        unclear += cc.unclear_winners(like, tg[t], groups)
    o.close()
    print("%s: %d trained groups, %d unclear winners" % (name, trained, unclear))
    assert trained > 0 and unclear == 0
