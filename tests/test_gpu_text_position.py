"""The text position of a stream (recur_amd/csrc/text_pos_rule.h) at its three device sites, each with the wrap taken and
on a sharded set: k_fwd_fused's tile (hidden 32: the plan gives k_fwd_fused<0>, the rolled form), k_assemble (hidden 33)
and k_bottom_forward (a bottom layer of 8 -> 6 under hidden 33).

A 9-byte text over an 8-symbol alphabet; the set holds streams 2 and 3 of 4, so the streams start 2 symbols apart and read
at i + 4 and i + 6, wrapped at 8: at i = 0 neither wraps, at i = 5 and at i = 7 both do.  The batched text step
(rnn_amd_set_char_step_deltas, position computed on the device) is held to the per-net driver's char_step_deltas
(recur_amd/drivers.py), which computes the position in Python and feeds each net its symbol through the reference's own
calls on the same library -- the independent statement of the rule.  The library refuses to TRAIN a bottom layer on a
sharded set (its error accumulator runs through the streams in order, recur-nn.c:377-382), so k_bottom_forward is reached
by the forward-only text step, rnn_amd_set_text_opinion with advance, and the target it leaves by the softmax error that
follows it; held to the per-net driver's rnn_bptt_advance + net_error_bptt of the symbol and its target at the reference's
position, (i + stream * spacing) % (len - 1)."""
import subprocess

import numpy as np
import pytest

import recur_ctypes as rc
import scenarios as sc
from test_fwd_plan import CXX as PLAN_CXX, SRC as PLAN_SRC, plan

gpu = pytest.mark.gpu
RTOL = 1e-4  # the parity tests' bound between two orders of the same float32 sums
TEXT = np.array([3, 1, 4, 1, 5, 2, 6, 5, 3], np.uint8)
SHARD = (2, 4)
POSITIONS = (0, 5, 7)
CASES = {
    "fused_tile": dict(input_size=8, hidden_size=32, output_size=8),
    "assemble": dict(input_size=8, hidden_size=33, output_size=8),
    "bottom_layer": dict(input_size=6, hidden_size=33, output_size=8, bottom_inputs=8),
}


@pytest.fixture(scope="module")
def amd():
    lib = rc.load_amd()
    assert lib.rnn_amd_device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return lib


def test_the_cases_wrap_where_the_docstring_says():
    last, spacing = len(TEXT) - 1, (len(TEXT) - 1) // SHARD[1]
    raw = {i: [i + (SHARD[0] + j) * spacing for j in range(2)] for i in POSITIONS}
    assert raw == {0: [4, 6], 5: [9, 11], 7: [11, 13]} and last == 8
    assert int(TEXT.max()) < 8  # symbols index 8 inputs


def test_the_plan_gives_each_case_the_site_it_is_named_after(tmp_path):
    """asked of fwd_plan.h itself, for the whole pass (want 0: rnn_amd_set_text_opinion) and for the text step's (want 1)"""
    exe = str(tmp_path / "fwd_plan_harness")
    subprocess.run(PLAN_CXX + [PLAN_SRC, "-o", exe], check=True)
    want = {"fused_tile": ("inside", "fused", 0, 1), "assemble": ("assemble", "gemm", 0, 0), "bottom_layer": ("bottom", "gemm", 0, 0)}
    for name, c in CASES.items():
        for w in (0, 1):
            p = plan(exe, input=c["input_size"], hidden=c["hidden_size"], output=c["output_size"], bottom=c.get("bottom_inputs", 0),
                     streams=2, mode=3, advance=1, want=w)
            # ns 0, one stage: k_fwd_fused<0>, the rolled form of the tile
            assert (p["input"], p["hidden"], p["ns"], p["nstages"]) == want[name], (name, w, p)


def symbol(i, j, ahead=0):
    """the symbol stream j of the shard reads at position i, at the reference's offset; ahead = 1: its target"""
    return int(TEXT[(i + (SHARD[0] + j) * ((len(TEXT) - 1) // SHARD[1])) % (len(TEXT) - 1) + ahead])


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_a_sharded_set_reads_the_text_where_the_per_net_driver_does(amd, name):
    kw = dict(CASES[name], S=2, D=3, learn_rate=1e-3, seed=19, shard=SHARD)
    orc = rc.load_oracle()
    g = sc.AmdBatchedSet(amd, **kw)
    g.load_text(TEXT)
    amd.rnn_amd_set_shard(g.handle, *SHARD)
    p = sc.ApiSet(amd, softmax_best_guess=orc.orc_softmax_best_guess, **kw)
    forward_only = "bottom_inputs" in kw
    keys = ["hist", "hidden", "output", "o_error"] + ([] if forward_only else ["ih_delta", "ho_delta"])
    for i in POSITIONS:
        if forward_only:
            amd.rnn_amd_set_text_opinion(g.handle, i, 1)
            amd.rnn_amd_set_softmax_error(g.handle, None)  # against the targets k_bottom_forward left: text[o + 1]
            for j in range(2):
                amd.rnn_bptt_advance(p.nets[j])
                p.net_error_bptt(j, symbol(i, j), symbol(i, j, 1))
        else:
            g.char_step_deltas(TEXT, i)
            p.char_step_deltas(TEXT, i)
        sg, sp = g.snapshot(), p.snapshot()
        bad = sc.compare(sg, sp, RTOL, keys=keys, exact=["index"])
        assert not bad, "i = %d: %s" % (i, "; ".join(bad))
        if not forward_only:  # the symbol itself, read off the one-hot input columns of the history slot the step filled
            for j in range(2):
                row = sg["hist"][sg["index"][j], j, kw["hidden_size"] + 1: kw["hidden_size"] + 1 + 8]
                assert np.array_equal(row, np.eye(8, dtype=np.float32)[symbol(i, j)]), (i, j, row)
    g.close()
    p.close()
