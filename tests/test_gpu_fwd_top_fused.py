"""The text step's forward pass and top layer as ONE launch (k_fwd_top, recur_amd/csrc/k_fwd_top.h) against the
two launches it replaces (k_fwd_fused + k_text_top2): bit identity, no tolerance.  Both forms run the same device bodies
(fwd_fused_tile, text_top2_rest), so every array and every statistic has to be equal bit for bit.

Twin sets from the same seed, each in a child process of its own (the library reads its switches once per process): one
with the one launch, where recur_amd/csrc/fwd_top_plan.h takes the call, one with RECUR_AMD_FWD_TOP=0.  Three
rnn_amd_set_char_step generations each, then every array of snapshot() and the statistics.  The library's own count of
one-launch text steps says which form ran in which process."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GENERATIONS = 3
# case -> hidden, streams of the training set, depth, symbols, activation (rnn_activation), first stream and size of the set
CASES = {
    "one_row_tile": dict(hidden=1024, streams=32, depth=3, symbols=42, activation=1),
    "two_xcds": dict(hidden=1024, streams=64, depth=3, symbols=42, activation=1),
    "wide_alphabet": dict(hidden=1024, streams=32, depth=3, symbols=64, activation=1),  # o_size 64: the softmax wave's edge
    "resqrt": dict(hidden=1024, streams=32, depth=3, symbols=42, activation=2),
    "reclip20": dict(hidden=1024, streams=32, depth=3, symbols=42, activation=5),
    "set_not_at_row_0": dict(hidden=1024, streams=64, depth=3, symbols=42, activation=1, first=32, count=32),
}


def run_case(name):
    """Three generations of the case; returns (arrays by name, one-launch text steps so far)."""
    sys.path.insert(0, HERE)
    import recur_ctypes as rc
    import scenarios as sc

    c = CASES[name]
    amd = rc.load_amd()
    amd.rnn_amd_fwd_top_launches.restype = C.c_long
    amd.rnn_amd_fwd_top_launches.argtypes = []
    before = amd.rnn_amd_fwd_top_launches()
    text = sc.synthetic_text(4000, alphabet=c["symbols"])
    full = sc.ApiSet(amd, c["symbols"], c["hidden"], c["symbols"], c["streams"], c["depth"], activation=c["activation"],
                     learn_rate=1e-3, seed=11)
    first, count = c.get("first", 0), c.get("count", c["streams"])
    nets = (type(full.nets[0]) * count)(*[full.nets[first + j] for j in range(count)])
    handle = amd.rnn_amd_set_open(nets, count)
    assert handle
    amd.rnn_amd_set_load_text(handle, rc.u8ptr(text), len(text))
    for i in range(GENERATIONS):
        amd.rnn_amd_set_char_step(handle, i, rc.WEIGHTED, 0.9)
    st = rc.AmdStats()
    amd.rnn_amd_set_read_stats(handle, C.byref(st), 0)
    out = dict(full.snapshot())
    for field, _ in st._fields_:
        out["stat_" + field] = np.asarray(getattr(st, field))
    amd.rnn_amd_set_close(handle)
    launches = amd.rnn_amd_fwd_top_launches() - before
    full.close()
    return out, launches


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_one_launch_equals_two_launches_bit_for_bit(name, tmp_path):
    # (both twins in processes of their own: whether the one launch takes a call also hangs on what the process has done
    # before -- a side stream opened, a residency probe that failed -- and a test process has done many things)
    twins = {}
    for switch in ("1", "0"):
        path = str(tmp_path / ("fwd_top_%s.npz" % switch))
        env = {k: v for k, v in os.environ.items() if not k.startswith("RECUR_AMD_")}
        env["RECUR_AMD_FWD_TOP"] = switch
        subprocess.run([sys.executable, os.path.abspath(__file__), name, path], env=env, check=True)
        twins[switch] = np.load(path)
    got, want = twins["1"], twins["0"]
    launches = int(got["one_launch_steps"])
    assert launches == GENERATIONS, "the one-launch form did not take the call (%d of %d text steps)" % (launches, GENERATIONS)
    assert int(want["one_launch_steps"]) == 0
    keys = sorted(k for k in want.files if k != "one_launch_steps")
    assert keys == sorted(k for k in got.files if k != "one_launch_steps") and "hidden" in keys and "stat_error" in keys
    bad = [k for k in keys if got[k].tobytes() != want[k].tobytes()]
    assert not bad, "not bit-identical: " + ", ".join(bad)


if __name__ == "__main__":  # the child: the same case with the switch as the environment has it
    arrays, n = run_case(sys.argv[1])
    np.savez(sys.argv[2], one_launch_steps=np.int64(n), **arrays)
