"""What tests/test_gpu_staggered_rings.py rests on, shown without a GPU:

  * the plan table: every case of staggered_cases.CASES, asked of chain_plan.h, calc_plan.h and fwd_plan.h through their
    harnesses with uniform_idx = -1, gets the forms the case is there for (k_chain_main<false> with the stages counted at
    run time, the generic delta GEMM small or big, assemble + GEMM with its planes left or finalized) -- and the two twin
    cases get the one-launch chain, the fused forward launch and k_delta_direct in lock step;
  * the oracle premise: a ring position is storage and nothing else -- a staggered and a lock-step set train bit-identical
    nets on the oracle;
  * the row rule restated in numpy agrees with the oracle's history, and each of three mutants of it picks another row
    than the rule somewhere in every case's set: the cases' staggers would notice those mistakes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import recur_ctypes as rc
import scenarios as sc
import staggered_cases as st
import test_calc_plan as calc
import test_chain_plan as chain
import test_fwd_plan as fwd

ROOT = rc.ROOT
CSRC = os.path.join(ROOT, "recur_amd", "csrc")


@pytest.fixture(scope="module")
def harnesses(tmp_path_factory):
    d = tmp_path_factory.mktemp("staggered_plans")
    exes = {}
    for name in ("chain", "calc", "fwd"):
        exes[name] = str(d / (name + "_plan_harness"))
        subprocess.run(chain.CXX + [os.path.join(ROOT, "tests", name + "_plan_harness.cpp"), "-o", exes[name]], check=True)
    return exes


@pytest.mark.parametrize("label", sorted(st.CASES))
def test_what_a_staggered_case_gets(harnesses, label):
    c = st.CASES[label]
    p = chain.plan(harnesses["chain"], **st.chain_args(c), uniform_idx=-1)
    chain.has(p, wanted=0, form="main", uniform=0, ns=0, mt=32, parts=c["chain"]["tn"], **c["chain"])
    chain.segments(p)
    p = calc.plan(harnesses["calc"], **st.calc_args(c), uniform_idx=-1)
    calc.has(p, direct=0, direct_runs=0, dma=0, has_rest=0, ho_in_delta=0, small=0, **c["calc"])
    p = fwd.plan(harnesses["fwd"], **st.fwd_args(c), uniform_idx=-1)
    fwd.has(p, hidden="gemm", uniform=0, noise="none", **c["fwd"])
    assert p["input"] != "inside"


@pytest.mark.parametrize("label", st.TWINS)
def test_what_a_twin_gets_in_lock_step(harnesses, label):
    c, want = st.CASES[label], st.TWIN_LOCK_STEP[label]
    chain.has(chain.plan(harnesses["chain"], **st.chain_args(c)), **want["chain"])
    calc.has(calc.plan(harnesses["calc"], **st.calc_args(c)), **want["calc"])
    fwd.has(fwd.plan(harnesses["fwd"], **st.fwd_args(c)), end="left", **want["fwd"])


def test_what_the_two_halves_get(harnesses):
    """hidden 256 / 64 streams / depth 6 as two sets of 32, each in lock step: a one-launch chain of two 16-stream tiles
    over its own rows (2 x 8 = 16 workgroups at work); as one set at two positions: k_chain_main<false>"""
    for row0 in (0, 32):
        p = chain.plan(harnesses["chain"], hidden=256, nrows=32, depth=6, row0=row0, scap=64)
        chain.has(p, wanted=1, windowed=0, uniform=1)
        chain.segments(p, "%d,32,1,0,32,0>240,1" % row0)
    p = chain.plan(harnesses["chain"], hidden=256, nrows=64, depth=6, uniform_idx=-1)
    chain.has(p, wanted=0, form="main", uniform=0, ns=0, nstages=2, tm=2, tn=8, blocks=16)
    chain.segments(p)


# ------------------------------------------------------------------------ the oracle premise --

def _oracle_run(kw, steps, staggered):
    o = sc.OracleSet(**kw)
    if staggered:
        st.stagger_oracle(o)
    text = sc.synthetic_text(6000)
    rows = []
    for i in range(steps):
        o.char_step(text, i, rc.WEIGHTED, 0.95)
        a = o.arrays()
        rows.append(np.stack([a["hist"][int(a["index"][j]), j].copy() for j in range(o.S)]))
    snap = o.snapshot()
    o.close()
    return snap, rows


def test_the_oracle_trains_the_same_net_wherever_the_rings_stand():
    """70 streams at hidden 40, depth 7, 12 generations, staggered and in lock step from the same seed on the same text:
    weights and momentum bit for bit, and the history too once every stream's ring is turned back by its offset.  The
    per-stream arithmetic and the order of the sum over streams do not depend on the slot, so the lock-step twins of the
    GPU tests compare two kernel families on the same mathematics."""
    kw = dict(input_size=42, hidden_size=40, output_size=42, S=70, D=7, learn_rate=1e-3, seed=3)
    stag, _ = _oracle_run(kw, 12, True)
    lock, _ = _oracle_run(kw, 12, False)
    off = st.stagger_offsets(70, 7)
    assert st.distinct_positions(stag["index"]) == 7 and st.distinct_positions(lock["index"]) == 1
    assert np.array_equal(stag["index"], (lock["index"] + off) % 7)
    for k in ("ih_w", "ho_w", "ih_m", "ho_m", "ih_delta", "ho_delta", "hidden", "output", "ih_scale", "min_error_factor"):
        assert np.array_equal(stag[k], lock[k]), k
    for j in range(70):
        assert np.array_equal(np.roll(stag["hist"][:, j], -int(off[j]), axis=0), lock["hist"][:, j]), j


# ------------------------------------------------------------------------------ the row rule --

def test_the_row_rule_agrees_with_the_oracles_history():
    """depth_wrap_64_33_9 on the oracle: after its warm-up the row the rule picks for (stream, steps back) holds what that
    stream's step wrote then, for every stream and every step of the ring"""
    c = st.CASES["depth_wrap_64_33_9"]
    kw = dict(c["kw"], learn_rate=1e-5, seed=3)
    D, S = kw["D"], kw["S"]
    snap, rows = _oracle_run(kw, D + 3, True)
    assert st.distinct_positions(snap["index"]) == 9
    idx = snap["index"].astype(np.int64)
    wrapped = 0
    for back in range(D):
        slot = st.slot_rule(idx, back, D)
        assert ((slot >= 0) & (slot < D)).all()
        wrapped += int((idx - back < 0).sum())
        got = snap["hist"][slot, np.arange(S)]
        assert np.array_equal(got, rows[-1 - back]), back
        if back:  # the rows are not all alike: picking another step's row would show
            assert not np.array_equal(got, rows[-back])
    assert wrapped == sum(int(D - 1 - i) for i in idx)


@pytest.mark.parametrize("label", sorted(st.CASES) + ["two_halves"])
@pytest.mark.parametrize("mutant", sorted(st.MUTANTS))
def test_a_wrong_row_rule_picks_another_row_in_every_case(label, mutant):
    """every mutant differs from the rule for some (stream, step back) of the set, whatever the number of generations the
    set has made since it was staggered"""
    if label == "two_halves":
        S, D = 64, 6
        base = np.where(np.arange(S) >= 32, 2, 0)
    else:
        S, D = st.CASES[label]["kw"]["S"], st.CASES[label]["kw"]["D"]
        base = st.stagger_offsets(S, D)
    for generations in range(D):
        idx = (base + generations) % D
        assert len(set(idx.tolist())) >= (2 if label == "two_halves" else min(D, S))
        differs = [(int(np.nonzero(d)[0][0]), back) for back in range(D)
                   for d in [st.MUTANTS[mutant](idx, back, D) != st.slot_rule(idx, back, D)] if d.any()]
        assert differs, "%s would pass %s after %d generations" % (mutant, label, generations)


def test_the_issues_own_stagger_where_three_divides_the_depth():
    """(3 j + 1) % D alone lands on D / 3 positions at depth 6, 9 and 12; extra_advances is that formula wherever it
    visits every position, and visits every position always"""
    for D in range(2, 21):
        for S in (1, 2, D - 1, D, 33, 70):
            if S < 1:
                continue
            off = st.stagger_offsets(S, D)
            assert st.distinct_positions(off) == min(D, S), (D, S)
            if D % 3:
                assert np.array_equal(off[:D], (3 * np.arange(S)[:D] + 1) % D)
    assert st.distinct_positions((3 * np.arange(33) + 1) % 9) == 3
