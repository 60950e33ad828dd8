"""The one-launch BPTT chain that starts each half-step's multiply while the previous half-step's row stores drain
(k_chain_persist_early, recur_amd/csrc/k_chain_persist.h) against the form without (k_chain_persist): bit identity, no
tolerance.  Both kernels are one text (k_chain_persist_body.h) and issue the same MFMAs into the same accumulators in the
same order; only where the wave stands when it issues the first eight differs.  The one outcome that would be silently
wrong -- a flag published in front of the drain, consumers fetching rows that have not arrived -- shows as different bits.

Twin sets from the same seed, each in a child process of its own (the library reads its switches once per process): one
with the early form, where recur_amd/csrc/chain_plan.h (chain_early_blocks) gives it, one with RECUR_AMD_CHAIN_EARLY=0.
Three rnn_amd_set_char_step generations each, then every array of snapshot() and the statistics.  The library's own count
of early-form launches says which kernel ran in which process.

The shapes are the smallest at which it can go wrong, one or two row tiles; sets that small run as 16-stream tiles by
default, which have no early form, so both twins run with RECUR_AMD_CHAIN_ONE=0: 32-stream tiles, the benchmark's kernel.

Depth 1: half-step 1 is the only one that finishes AND multiplies, half-step 2 only finishes; depth 2 and 3 add the
steady state.  64 streams: two row tiles, two XCDs.  RESQRT and RECLIP20: the finish divides and clips in front of the
stores.  A 32-stream set at row 32 of 64: the launch does not start at row 0.

The twins could be wrong together, so one case holds the early form to the per-net driver (recur_amd/drivers.py: the
reference's own calls, net by net, whose chains are 16-stream padded launches of k_chain_persist) at the parity tests' bar."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GENERATIONS = 3
RTOL = 1e-4  # the parity tests' bound between two orders of the same float32 sums
# case -> hidden, streams of the training set, depth, symbols, activation (rnn_activation), first stream and size of the set
CASES = {
    "depth_1": dict(hidden=1024, streams=32, depth=1, symbols=42, activation=1),
    "depth_2": dict(hidden=1024, streams=32, depth=2, symbols=42, activation=1),
    "depth_3": dict(hidden=1024, streams=32, depth=3, symbols=42, activation=1),
    "two_xcds": dict(hidden=1024, streams=64, depth=3, symbols=42, activation=1),
    "resqrt": dict(hidden=1024, streams=32, depth=3, symbols=42, activation=2),
    "reclip20": dict(hidden=1024, streams=32, depth=3, symbols=42, activation=5),
    "set_not_at_row_0": dict(hidden=1024, streams=64, depth=3, symbols=42, activation=1, first=32, count=32),
}


def early_count(amd):
    amd.rnn_amd_chain_early_launches.restype = C.c_long
    amd.rnn_amd_chain_early_launches.argtypes = []
    return amd.rnn_amd_chain_early_launches()


def run_case(name):
    """Three generations of the case; returns (arrays by name, early-form chain launches so far)."""
    sys.path.insert(0, HERE)
    import recur_ctypes as rc
    import scenarios as sc

    c = CASES[name]
    amd = rc.load_amd()
    before = early_count(amd)
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
    launches = early_count(amd) - before
    full.close()
    return out, launches


def run_against_the_per_net_driver():
    """32 streams, depth 3, RELU: the batched text step (early form) and the per-net driver side by side; returns the
    mismatches and the early-form launches of the batched set's steps."""
    sys.path.insert(0, HERE)
    import recur_ctypes as rc
    import scenarios as sc

    amd = rc.load_amd()
    orc = rc.load_oracle()
    kw = dict(input_size=42, hidden_size=1024, output_size=42, S=32, D=3, learn_rate=1e-3, seed=19)
    text = sc.synthetic_text(4000)
    g = sc.AmdBatchedSet(amd, **kw)
    g.load_text(text)
    p = sc.ApiSet(amd, softmax_best_guess=orc.orc_softmax_best_guess, **kw)
    bad, launches = [], 0
    for i in range(GENERATIONS):
        before = early_count(amd)
        g.char_step_deltas(text, i)
        amd.rnn_amd_synchronize()
        launches += early_count(amd) - before
        p.char_step_deltas(text, i)
        bad += ["i = %d: %s" % (i, b) for b in sc.compare(g.snapshot(), p.snapshot(), RTOL,
                                                            keys=["hist", "hidden", "output", "o_error", "ih_delta", "ho_delta"],
                                                            exact=["index"])]
    g.close()
    p.close()
    return bad, launches


def child(args, switch):
    env = {k: v for k, v in os.environ.items() if not k.startswith("RECUR_AMD_")}
    env["RECUR_AMD_CHAIN_EARLY"] = switch
    env["RECUR_AMD_CHAIN_ONE"] = "0"  # 32-stream row tiles for these small sets too (by default up to 128 streams run as 16-stream tiles)
    return subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, check=True, capture_output=True, text=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_early_form_equals_the_chain_without_bit_for_bit(name, tmp_path):
    # (both twins in processes of their own: whether the one-launch chain takes a call also hangs on what the process has
    # done before -- a side stream opened, a residency probe that failed -- and a test process has done many things)
    twins = {}
    for switch in ("1", "0"):
        path = str(tmp_path / ("chain_early_%s.npz" % switch))
        child([name, path], switch)
        twins[switch] = np.load(path)
    got, want = twins["1"], twins["0"]
    launches = int(got["early_launches"])
    assert launches == GENERATIONS, "the early form did not take the call (%d of %d chain launches)" % (launches, GENERATIONS)
    assert int(want["early_launches"]) == 0
    keys = sorted(k for k in want.files if k != "early_launches")
    assert keys == sorted(k for k in got.files if k != "early_launches") and "hidden" in keys and "stat_error" in keys
    bad = [k for k in keys if got[k].tobytes() != want[k].tobytes()]
    assert not bad, "not bit-identical: " + ", ".join(bad)


@pytest.mark.gpu
def test_the_early_form_holds_to_the_per_net_driver():
    out = child(["--per-net"], "1").stdout.strip().splitlines()
    assert out and out[-1] == "early_launches=%d mismatches=0" % GENERATIONS, "\n".join(out)


if __name__ == "__main__":  # the child: the same case with the switch as the environment has it
    if sys.argv[1] == "--per-net":
        mismatches, n = run_against_the_per_net_driver()
        for line in mismatches:
            print(line)
        print("early_launches=%d mismatches=%d" % (n, len(mismatches)))
    else:
        arrays, n = run_case(sys.argv[1])
        np.savez(sys.argv[2], early_launches=np.int64(n), **arrays)
