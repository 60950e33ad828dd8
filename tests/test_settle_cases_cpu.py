"""What tests/test_gpu_settle.py rests on, shown without a GPU (tests/settle_cases.py):

  * every script passes the budget of exact_cases.py at LIMIT_BITS: no sum of it can round in any order, so one snapshot
    at the end owes the reference every element (the output layer behind the update excepted, as in the exact-generation
    tests: it is asserted to be over the limit);
  * the oracle (float32, the reference's own order) equals the restatement at the end of the script on every array, bit
    for bit.  ON THE ORACLE: every script of "ragged", "ranged" and "masked", and `apply_takes_planes` (all three methods) and
    `accumulate_on_planes` of "h256" and "h512" (settle_cases.ON_THE_ORACLE); the other scripts of the two larger nets
    are the same restated operations, which the small nets' scripts and tests/test_exact_cases_cpu.py pin;
  * every script can tell right from wrong: each wrong settlement it names, restated, changes the final snapshot in at
    least one of ih_w, ho_w, ih_delta, ho_delta, err_a;
  * the producer of every planes script gets the `planes` forms from calc_plan.h, with the workspace the engine passes, and
    those forms are the planes the scripts' deferred bits expect;
  * the scripts' shape: a producer first, `update, forward` last, at most two generations summed."""
import functools
import os
import subprocess

import numpy as np
import pytest

import exact_cases as ec
import recur_ctypes as rc
import settle_cases as st
import test_calc_plan as calc
import test_chain_plan as chain

ALL_KEYS = ec.FLOAT_KEYS + ec.INT_KEYS + ("err_b", "top_error_raw", "top_error_scaled")
TELLING = ("ih_w", "ho_w", "ih_delta", "ho_delta", "err_a")


@functools.lru_cache(maxsize=None)
def right(case_name, script_name):
    """-> (the RestatedDriver with its budget, its final snapshot), once per script"""
    d = st.restated(case_name, script_name, budget=ec.Budget())
    return d, d.snapshot()


@pytest.mark.parametrize("case_name,script_name", st.PAIRS)
def test_the_budget_holds(case_name, script_name):
    b = right(case_name, script_name)[0].r.budget
    print("%s, %s: %s" % (case_name, script_name, ", ".join("%s %.1f" % kv for kv in sorted(b.bits.items()))))
    assert not b.failed, b.failed
    assert b.over(ec.GENERATION + ("hidden after",)) == [], b.over()
    assert b.over(("output after",)) == ["output after"], "the output layer behind the update fits after all"


@pytest.mark.parametrize("case_name,script_name", st.ON_THE_ORACLE)
def test_the_oracle_equals_the_restatement(case_name, script_name):
    d, want = right(case_name, script_name)
    got = st.on_the_oracle(case_name, script_name)
    keys = tuple(k for k in ALL_KEYS if k != "output")
    assert ec.first_difference(got, want, keys) is None, ec.first_difference(got, want, keys)
    assert (np.abs(got["output"] - d.r.output) <= ec.rounded_output_bound(d.r)).all()


def test_every_script_runs_on_the_oracle_on_some_net():
    assert {s for _, s in st.ON_THE_ORACLE} == {s for _, s in st.PAIRS}
    assert all((n, s) in st.ON_THE_ORACLE for n, s in st.PAIRS if n in ("ragged", "ranged", "masked"))


@pytest.mark.parametrize("case_name,script_name", st.PAIRS)
def test_the_script_can_tell_right_from_wrong(case_name, script_name):
    _, want = right(case_name, script_name)
    s = st.script(case_name, script_name)
    assert s.wrong
    for wrong in s.wrong:
        bad = st.restated(case_name, script_name, wrong=wrong).snapshot()
        seen = ec.differences(bad, want)
        print("%s, %s, %s: %s" % (case_name, script_name, wrong, "; ".join(seen) or "NOT SEEN"))
        assert seen, "%s would pass %s on %s" % (wrong, script_name, case_name)
        assert any(line.split(":")[0] in TELLING for line in seen), seen


def test_the_wrong_settlements_of_the_issue_are_all_somebodys():
    for scripts in (st.PLANE_SCRIPTS, st.RANGED_SCRIPTS, st.MASKED_SCRIPTS):
        named = {w for s in scripts for w in s.wrong}
        assert named >= (set(st.WRONG) - {"images_zeroed"} if scripts is st.PLANE_SCRIPTS else {"images_zeroed"})


def test_clear_drops_planes_reads_back_zeros_and_moves_by_momentum_alone():
    d, snap = right("ragged", "clear_drops_planes")
    assert not snap["ih_delta"].any() and not snap["ho_delta"].any()
    net = ec.net_of(d.c)
    assert np.array_equal(snap["ih_w"], np.float32(net["ih_w"] + net["ih_m"] * ec.MOMENTUM))    # (NESTEROV: w + momentum m)
    assert st.restated("ragged", "apply_takes_planes[NESTEROV]").r.ih_delta.any()


# ------------------------------------------------------------------------------------------- the plan table --

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("settle_plans") / "calc_plan_harness")
    subprocess.run(chain.CXX + [os.path.join(rc.ROOT, "tests", "calc_plan_harness.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("case_name", list(st.SCRIPTS))
def test_the_producer_leaves_the_planes_the_bits_expect(harness, case_name):
    """rnn_amd_set_calc_deltas(accumulate 0) of each case, with the engine's own workspace of 8 I H + 64 x 128 H floats:
    the case's `planes` forms; ih planes unless one workgroup or the GEMM's own epilogue does it all, ho planes where the
    top delta's GEMM leaves planes"""
    c = st.CASES[case_name]
    f = c["forms"]
    calc_args = ec.plan_args(c, "planes")[0]
    I, H, _ = ec.padded(c["input_size"], c["hidden_size"], c["output_size"])
    assert calc_args["defer"] == 1 and calc_args["accumulate"] == 0 and calc_args["own_slab_floats"] == 8 * I * H + 64 * 128 * H
    p = calc.plan(harness, **calc_args)
    calc.has(p, **dict(f.get("calc", {}), **f.get("planes", {})))
    got = (st.IH_PLANES if not p["small"] and not p["direct_fuse"] else 0) | \
          (st.HO_PLANES if p["ho_gemm"] in ("planes", "planes_paired") else 0)
    assert got == st.PLANES[case_name]
    # ... and the per-net call on one stream of the small net is k_bptt_small: one workgroup, no workspace, no planes
    if case_name == "ragged":
        one = dict(calc_args, streams=1, defer=0, accumulate=1)
        one.pop("own_slab_floats")
        calc.has(calc.plan(harness, **one), small=1)


# ------------------------------------------------------------------------------------------- the scripts' shape --

def test_the_shape_of_the_scripts():
    for case_name, scripts in st.SCRIPTS.items():
        assert len({s.name for s in scripts}) == len(scripts)
        for s in scripts:
            ops = [op for op, _ in s.ops]
            assert ops[0][0] == "delta" and ops[-2:] == [("update",), ("forward", 2)]
            assert all(letters is not None and set(letters) <= set("PCE") for _, letters in s.ops[:-1])
            # planes are expected only behind a set call that does not accumulate -- or absorbs a clear
            for i, (op, letters) in enumerate(s.ops[:-1]):
                if op[0] == "delta" and (op[2] == 0 or (i > 0 and "C" in s.ops[i - 1][1])):
                    assert "P" in letters, (s.name, op)
            assert st.bits(case_name, s.ops[0][1], keep=False) & (st.IH_PLANES | st.HO_PLANES) == 0
    assert [s.method for s in st.PLANE_SCRIPTS[:3]] == ["WEIGHTED", "NESTEROV", "CLASSICAL"]
