"""What tests/test_gpu_exact_generations.py rests on, shown without a GPU, from the oracle alone (tests/exact_cases.py):

  * the budget: every sum of every case is a sum of integers times a power of two that fits 24 bits with one to spare --
    the condition under which no order of summation can round.  The table of bits used is printed.  The one stage that does
    not fit is the OUTPUT layer of the forward pass behind the update (two fine grids multiplied): it is asserted to be
    over the limit, so that holding it at a rounding bound instead of bit for bit is the condition's verdict, not a habit;
  * the oracle (float32, in the reference's own order) equals the float64 restatement on every array, bit for bit;
  * the decisions the chain takes are not close calls: no stream is scaled, the top error is at most half its clip, every
    executed step's sum of squares is at most half the ceiling and either exactly 0 or more than twice the exit threshold;
  * the gates are exercised: zeros, non-zeros and (RECLIP20) units at exactly 20.0 in the history; two or more executed
    depths per dyadic case, one of them the zero row's;
  * the zero-answer nets answer exactly 0, their likelihoods are exactly 1 / n, their hidden errors are not zero -- and
    cancel in the first chain step (twin columns, opposite errors), so that their chain ends there: depth 0 on every stream;
  * every case gets the launch forms it is in the table for (calc_plan.h, chain_plan.h, fwd_plan.h through their harnesses);
  * each of six broken rules makes the restatement differ from the oracle on every case it applies to."""
import functools
import os
import subprocess

import numpy as np
import pytest

import exact_cases as ec
import recur_ctypes as rc
import test_calc_plan as calc
import test_chain_plan as chain
import test_fwd_plan as fwd

ROOT = rc.ROOT
ALL_KEYS = ec.FLOAT_KEYS + ec.INT_KEYS + ("err_b", "top_error_raw", "top_error_scaled")


@functools.lru_cache(maxsize=None)
def runs(name):
    """-> (the Restated with its budget, its snapshots, the oracle's snapshots), once per case"""
    c = ec.CASES[name]
    r, snaps = ec.restated_run(c, budget=ec.Budget())
    return r, snaps, ec.oracle_run(c)


def output_is_rounded(name, i):
    """the step is the forward pass behind the update, whose output layer the budget does not cover"""
    return ec.steps(ec.CASES[name])[i] == ec.steps(ec.CASES[name])[-1]


# ------------------------------------------------------------------------------------------------- the budget --

def test_the_budget_holds_and_here_is_the_table():
    stages = ec.GENERATION + ec.FORWARD_AFTER
    print()
    print("bits used per sum (limit %d)" % ec.LIMIT_BITS)
    print("%-12s" % "case" + "".join("%14s" % s for s in stages))
    for name in ec.CASES:
        b = runs(name)[0].budget
        print("%-12s" % name + "".join("%14s" % ("%.1f" % b.bits[s] if s in b.bits else "-") for s in stages))
        assert not b.failed, (name, b.failed)
        assert b.over(ec.GENERATION + ("hidden after",)) == [], (name, b.over())
        assert b.over(("output after",)) == ["output after"], "%s: the output layer behind the update fits after all" % name


def test_the_budget_notices_a_sum_that_does_not_fit():
    b = ec.Budget()
    b.dot("fits", np.full((1, 2 ** 13), 2.0 ** -10), np.full((2 ** 13, 1), 2.0 ** 10))      # 2^13 on a grid of 2^-10
    b.dot("too long", np.full((1, 2 ** 13), 3 * 2.0 ** -10), np.full((2 ** 13, 1), 2.0 ** 10))
    b.dot("no grid", np.array([[1.0 / 3]]), np.array([[1.0]]))
    assert b.bits["fits"] == 23.0 and b.over() == ["too long", "no grid: an operand is on no dyadic grid"]


# --------------------------------------------------------------------------------- the oracle and the restatement --

@pytest.mark.parametrize("name", list(ec.CASES))
def test_the_oracle_equals_the_restatement(name):
    r, snaps, want = runs(name)
    assert len(snaps) == len(want) == len(ec.steps(ec.CASES[name]))
    for i, (a, o) in enumerate(zip(snaps, want)):
        keys = tuple(k for k in ALL_KEYS if not (k == "output" and output_is_rounded(name, i)))
        assert ec.first_difference(o, a, keys) is None, "%s after %s: %s" % (name, ec.steps(ec.CASES[name])[i], ec.first_difference(o, a, keys))
    # the output layer behind the update, within the bound of a float32 sum of H terms in any order
    bound = ec.rounded_output_bound(r)
    assert (np.abs(want[-1]["output"] - r.output) <= bound).all()
    print("%s: the output layer behind the update may round by up to %.3g of its largest element" % (
        name, bound.max() / np.abs(r.output).max()))


# ---------------------------------------------------------------------------------------- no close calls --

@pytest.mark.parametrize("name", list(ec.CASES))
def test_the_decisions_are_not_close_calls(name):
    c = ec.CASES[name]
    r, snaps, want = runs(name)
    for o in want:
        assert (o["ih_scale"] == 1.0).all()
        assert (o["top_error_raw"] <= c["hidden_size"]).all()          # half the clip of 2 h_size
        assert np.array_equal(o["top_error_raw"], o["top_error_scaled"])
    assert r.margins and r.finals
    for s, step, sq, ceiling, low, give_up in r.margins:
        # (under error ranges a stream whose error row is zero still carries last time's entries of its idle units -- the
        # reference's own quirk, restated -- so its sums are measured against what decides: the give-up threshold
        # 2 top + 1 at every step, the ceiling at the last)
        assert sq <= 0.5 * (give_up if c["ranges"] else ceiling), (name, s, step, sq, ceiling)
        assert sq == 0 or sq > 2 * low, (name, s, step, sq, low)
    for s, sq, ceiling in r.finals:
        assert sq <= 0.5 * ceiling, (name, s, sq, ceiling)


@pytest.mark.parametrize("name", list(ec.CASES))
def test_the_gates_are_exercised(name):
    c = ec.CASES[name]
    _, _, want = runs(name)
    hs = c["hidden_size"]
    for o in want:
        h = o["hidden"][:, 1:1 + hs]
        assert (h == 0).mean() >= 0.25 and (h != 0).mean() >= 0.25, (name, (h == 0).mean())
    trained = [o for (what, _), o in zip(ec.steps(c), want) if what in ("delta", "step")]
    if c["activation"] == ec.RECLIP20:
        assert any((o["hist"] == 20.0).any() for o in trained), "%s: no unit at the ceiling" % name
    depths = set()
    for (what, g), o in zip(ec.steps(c), trained):
        depths |= set(o["bptt_depth"].tolist())
    if c["kind"] == "dyadic":
        assert len(depths) >= 2 and 0 in depths and c["D"] in depths, (name, depths)
        for g, o in enumerate(trained):
            zero = [s for s in range(c["S"]) if ec.row_kind(c, g, s) == 0 and ec.active_mask(c, g)[s]]
            assert zero or c["S"] == 1 or c["masked"]
            assert all(not o["o_error"][s].any() for s in zero)
            # (under error ranges the idle units' entries of last time run on: the depth is theirs)
            assert c["ranges"] or all(o["bptt_depth"][s] == 0 for s in zero)
    else:
        assert depths == {0}    # the twins' errors cancel in the first step: see the module docstring


@pytest.mark.parametrize("name", ec.DYADIC)
def test_the_special_rows_are_what_they_claim(name):
    """a row that is non-zero only where W_ho's column is zero: a top delta, no hidden error"""
    c = ec.CASES[name]
    if c["ranges"]:
        return
    net = ec.dyadic_net(c)
    assert not net["ho_w"][:, list(net["zero_cols"])].any()
    seen = 0
    for g in range(ec.generations(c)):
        e = ec.error_rows(c, g, net["zero_cols"])
        for s in range(c["S"]):
            if ec.row_kind(c, g, s) == 1:
                assert e[s].any() and not (e[s] @ net["ho_w"].T.astype(np.float32)).any()
                seen += 1
    assert seen


@pytest.mark.parametrize("name", ec.ZERO_ANSWER)
def test_the_zero_answer_nets_answer_zero(name):
    c = ec.CASES[name]
    r, _, want = runs(name)
    n, hs, S = c["output_size"], c["hidden_size"], c["S"]
    step = [i for i, (what, _) in enumerate(ec.steps(c)) if what == "step"][0]
    gen = ec.steps(c)[step][1]
    for i, o in enumerate(want[:step + 1]):
        assert c["kind"] == "sigmoid" and i == step or (o["output"] == 0.0).all()
        assert np.array_equal(o["hidden"][:, 1:hs + 1:2], o["hidden"][:, 2:hs + 2:2])       # the twins
    o = want[step]
    trained = np.ones(S, bool)
    if c["kind"] in ("text", "fused"):   # every likelihood is exactly 1 / n
        _, tgt = ec.text_taps(ec.text_of(c), gen, S)
        like = -o["o_error"][:, :n].copy()
        like[np.arange(S), tgt] += 1
        assert (like == np.float32(1.0 / n)).all()
    elif c["kind"] == "heads":       # every trained head's likelihoods are exactly 1 / 32; the others have no error
        e, cols = ec.head_errors(c, gen)
        A = c["input_size"]
        _, nxt, cls = ec.head_inputs(c, gen)
        assert np.array_equal(o["o_error"], e.astype(np.float32))
        assert len(set(cls.tolist())) == n // A       # every head is some stream's own
        assert cols.reshape(S, -1)[:, :n].reshape(S, n // A, A).all(axis=2).sum() == (S * (n // A) if c["leakage"] else S)
        for s in range(S):
            like = -o["o_error"][s, cls[s] * A:(cls[s] + 1) * A].copy()
            like[nxt[s]] += 1
            assert (like == np.float32(1.0 / A)).all()
    elif c["kind"] == "sigmoid":     # every answer is exactly 1 / 2, the error 1 / 4 (t - 1 / 2)
        assert (o["output"][:, :n] == 0.5).all() and not o["output"][:, n:].any()
        assert np.array_equal(o["o_error"][:, :n], np.float32(0.25) * (ec.sigmoid_targets(c, gen) - np.float32(0.5)))
        assert set(np.unique(o["o_error"][:, :n])) == {-0.125, -0.0625, 0.125}
    else:                            # every group's likelihoods are exactly 1 / its size, weighted
        e, mask, groups, wins, wrong = ec.group_errors(c, gen)
        trained = mask.astype(bool)
        assert np.array_equal(o["o_error"], e.astype(np.float32))
        assert 0 < trained.sum() < S and groups == (ec.group_targets(c, gen) >= 0).sum() and 0 < wins < groups
        goff, gsize = ec.group_layout()
        w = ec.group_weights(c)
        t = ec.group_targets(c, gen)
        for s in np.nonzero(trained)[0]:
            for g0, gn, tg in zip(goff, gsize, t[s]):
                like = -o["o_error"][s, g0:g0 + gn] / w[g0:g0 + gn]
                if tg >= 0:
                    like[tg] += 1
                assert (like == (np.float32(1.0 / gn) if tg >= 0 else 0)).all()
        assert set(np.unique(w[:n])) == {0.5, 1.0, 2.0}
    net = ec.zero_answer_net(c)
    herr = (o["o_error"].astype(np.float64) @ net["ho_w"].T)[:, 1:hs + 1:2]
    live = (o["hidden"][:, 1:hs + 1:2] != 0) & trained[:, None]
    assert (herr[live] != 0).mean() >= 0.5
    assert not np.array_equal(want[-1]["hidden"][:, 1:hs + 1:2], want[-1]["hidden"][:, 2:hs + 2:2])  # ... and then diverge


# ------------------------------------------------------------------------------------------- the plan table --

@pytest.fixture(scope="module")
def harnesses(tmp_path_factory):
    d = tmp_path_factory.mktemp("exact_plans")
    exes = {}
    for name in ("chain", "calc", "fwd"):
        exes[name] = str(d / (name + "_plan_harness"))
        subprocess.run(chain.CXX + [os.path.join(ROOT, "tests", name + "_plan_harness.cpp"), "-o", exes[name]], check=True)
    return exes


@pytest.mark.parametrize("name", list(ec.CASES))
def test_what_a_case_gets(harnesses, name):
    c = ec.CASES[name]
    f = c["forms"]
    for form in ("planes", "summed"):
        calc_args, chain_args, fwd_args = ec.plan_args(c, form)
        calc.has(calc.plan(harnesses["calc"], **calc_args), **dict(f.get("calc", {}), **f.get(form, {})))
    if "chain" in f:
        chain.has(chain.plan(harnesses["chain"], **chain_args), **f["chain"])
    fwd.has(fwd.plan(harnesses["fwd"], **fwd_args), **f["fwd"])


# -------------------------------------------------------------------------------- one broken rule at a time --

def applies(c, mutation):
    if mutation == "clipped_unit_live":
        return c["activation"] == ec.RECLIP20
    if c["kind"] != "dyadic":
        # a zero-answer chain ends in its first step with errors that cancel to 0: no deeper step, no second step to leave
        # a column out of, and the zero the first column would keep is a zero
        return mutation in ("stream_left_out_of_ho_delta",)
    return True


@pytest.mark.parametrize("mutation", ec.MUTATIONS)
@pytest.mark.parametrize("name", list(ec.CASES))
def test_a_broken_rule_is_noticed(name, mutation):
    c = ec.CASES[name]
    if not applies(c, mutation):
        return
    _, good, want = runs(name)
    trained = [i for i, (what, _) in enumerate(ec.steps(c)) if what in ("delta", "step")]
    _, bad = ec.restated_run(c, mutation=mutation, upto=trained[-1] + 1)
    first = next((i for i in trained if ec.first_difference(want[i], bad[i]) is not None), None)
    assert first is not None, "%s would pass %s" % (mutation, name)
    print("%s, %s: first seen after %s: %s" % (name, mutation, ec.steps(c)[first], ec.first_difference(want[first], bad[first])))
