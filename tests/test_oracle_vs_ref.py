"""Cross-check of the oracle against the real reference library over a run: the reference's struct sizes and its
state after a run, recorded from the compiled reference (tests/golden/ref_live.npz, tests/golden/make_golden_live.py).
The golden vectors of test_oracle_golden.py pin the oracle's single operations; this pins a whole training run."""
import numpy as np
import pytest

import golden_cases as gc
import recur_ctypes as rc
import scenarios as sc

Z = np.load(gc.LIVE_GOLDEN)


def ref_snapshot(prefix):
    return {k[len(prefix):]: Z[k] for k in Z.files if k.startswith(prefix)}


def test_abi_struct_sizes_match_reference():
    import ctypes as C
    assert int(Z["sizeof_net"]) == C.sizeof(rc.RecurNN)
    assert int(Z["sizeof_bptt"]) == C.sizeof(rc.RecurNNBPTT)


@pytest.mark.parametrize("act", [rc.RELU, rc.RESQRT, rc.RECLIP20])
@pytest.mark.parametrize("method", [rc.WEIGHTED, rc.NESTEROV])
def test_oracle_tracks_reference_over_a_run(act, method):
    an = {v: k for k, v in gc.RUN_ACTS.items()}[act]
    mn = {v: k for k, v in gc.RUN_METHODS.items()}[method]
    text = sc.synthetic_text(gc.RUN_TEXT_LEN)
    o = sc.OracleSet(activation=act, **gc.RUN_KW)
    start, end = ref_snapshot("run.start."), ref_snapshot("run.%s.%s.end." % (an, mn))
    snap = o.snapshot()
    assert set(start) == set(end) == set(sc.FLOAT_KEYS + sc.EXACT_KEYS) & set(snap)  # every array compared
    assert sc.compare(snap, start, 0) == []  # initialisation is bit-exact
    for i in range(gc.RUN_GENERATIONS):
        o.char_step(text, i, method, gc.RUN_MOMENTUM)
    assert sc.compare(o.snapshot(), end, 2e-6) == []
    o.close()
