"""The rest rows of k_delta_direct (the rows of ih_delta above the last whole 64-row tile: hidden unit 1024, the one-hot
input columns, the pad) against the oracle, at the smallest shapes each form of their pieces takes.

A workgroup's piece is (row group, column group mt % 4 of the error quad); the column group reaches the seventeenth MFMA as
a dword load of its own at the quad's per-lane offset + mt % 4 floats (k_delta_direct.h).  A wrong offset would put a
column group's sums into another's columns: every piece of a column tile is compared, rest rows on their own so that
44 rows cannot hide among 1024, over D + 3 generations (every slot of the history ring rewritten, the ring wrapped):

  * one piece per workgroup, four row groups (42 symbols: 44 rest rows), 32 streams / depth 5: one ring round per wave;
  * two pieces per workgroup, eight row groups (100 input columns: 104 rest rows);
  * two pieces per workgroup, four row groups, K split four ways over workgroups (hidden 512: 8 x 8 tiles)."""
import numpy as np
import pytest

import recur_ctypes as rc
import replay
import scenarios as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    lib = rc.load_amd()
    assert lib.rnn_amd_device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return lib


@pytest.mark.parametrize("hidden,inputs,S,D", [(1024, 42, 32, 5), (1024, 100, 32, 5), (512, 42, 128, 5)])
def test_rest_rows_of_the_direct_delta_gemm_match_the_oracle(amd, hidden, inputs, S, D):
    kw = dict(input_size=inputs, hidden_size=hidden, output_size=42, S=S, D=D, learn_rate=1e-3, seed=9)
    text = sc.synthetic_text(6000)
    g = sc.AmdBatchedSet(amd, **kw)
    o = sc.OracleSet(**kw)
    for i in range(D + 3):
        g.char_step(text, i, rc.WEIGHTED, 0.9)
        o.char_step(text, i, rc.WEIGHTED, 0.9)
        sg, so = g.snapshot(), o.snapshot()
        assert (so["ih_scale"] == 1.0).all()  # (the all-ones loop's regime; the hot one: test_gpu_parity.py)
        first_rest = hidden  # (row 0 is the bias: the tiles end with hidden unit `hidden` - 1)
        assert so["ih_delta"].shape[0] - first_rest > inputs
        for k in ("ih_delta", "ih_w", "ih_m"):
            sg[k + "_rest"], so[k + "_rest"] = sg[k][first_rest:], so[k][first_rest:]
            assert np.abs(so[k + "_rest"]).max() > 0
        replay.check(sg, so, 1e-4, keys=["ih_delta", "ih_w", "ih_m", "ih_delta_rest", "ih_w_rest", "ih_m_rest", "ho_w"])
    g.close()
    o.close()
