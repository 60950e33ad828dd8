"""How rnn_amd_run_texts lays a batch of texts over state rows, asked of the rule itself (recur_amd/csrc/texts_plan.h)
without a GPU: texts_plan_harness.c is compiled with the host compiler alone and prints the plan for the lengths, skips
and wave width on its command line.  And the refusals of the calls, which come before anything needs a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import recur_ctypes as rc

ROOT = rc.ROOT
CSRC = os.path.join(ROOT, "recur_amd", "csrc")
LENS = [5, 0, 2, 600, 1, 2, 64, 600]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("texts_plan") / "texts_plan_harness")
    subprocess.run(["gcc", "-std=gnu11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "texts_plan_harness.c"), "-o", exe], check=True)
    return exe


def plan(exe, width, lens, skips=None):
    args = [exe, str(width), ",".join(map(str, lens))]
    if skips is not None:
        args.append(",".join(map(str, skips)))
    out = subprocess.run(args, capture_output=True, text=True, check=True).stdout
    d = dict(line.split("=", 1) for line in out.splitlines())
    return {k: [int(x) for x in v.split(",")] if v else [] for k, v in d.items()}


def brute_active(lens, t):
    return sum(1 for n in lens if n - 1 > t)


def test_the_header_is_plain_c_and_cxx_without_hip():
    for cc, lang in (("gcc", "c"), ("g++", "c++")):
        subprocess.run([cc, "-fsyntax-only", "-Wall", "-Werror", "-Wno-unused-function", "-I", CSRC, "-x", lang,
                        os.path.join(CSRC, "texts_plan.h")], check=True)


def test_order_is_longest_first_stable_and_the_permutation_maps_back(harness):
    skips = [10, 11, 12, 13, 14, 15, 16, 17]
    p = plan(harness, 256, LENS, skips)
    assert p["n_rows"] == [6]                      # lengths 0 and 1 take no row
    assert p["order"] == [3, 7, 6, 0, 2, 5]        # 600, 600 (caller's order), 64, 5, 2, 2 (caller's order)
    assert p["len"] == [LENS[k] for k in p["order"]] == [600, 600, 64, 5, 2, 2]
    assert p["skip"] == [skips[k] for k in p["order"]]
    assert plan(harness, 256, LENS)["skip"] == [0] * 6  # no skips: zeros
    # results in plan order go back to the caller's places; the dropped texts keep their zero
    back = np.zeros(len(LENS), int)
    back[p["order"]] = p["len"]
    assert list(back) == [n if n >= 2 else 0 for n in LENS]


@pytest.mark.parametrize("width", [256, 3, 1])
def test_active_counts_are_the_brute_force_counts(harness, width):
    rng = np.random.default_rng(5)
    for lens in (LENS, [int(x) for x in rng.integers(0, 41, 50)]):
        p = plan(harness, width, lens)
        for w in range(p["n_waves"][0]):
            row0, nrows, steps = p["wave%d" % w]
            mine = p["len"][row0:row0 + nrows]
            a = p["active%d" % w]
            assert steps == max(mine) - 1 and len(a) == steps + 1
            assert a[:steps] == [brute_active(mine, t) for t in range(steps)]
            assert all(x >= y for x, y in zip(a, a[1:]))     # the active rows are a shrinking prefix
            assert a[0] == nrows and a[steps - 1] >= 1 and a[steps] == 0


def test_waves(harness):
    p = plan(harness, 3, [9, 8, 7, 6, 5, 4, 3, 2])
    assert p["n_waves"] == [3]
    assert [p["wave%d" % w] for w in range(3)] == [[0, 3, 8], [3, 3, 5], [6, 2, 2]]   # row0, rows, steps = longest - 1
    for width in (8, 9, 256):
        q = plan(harness, width, [9, 8, 7, 6, 5, 4, 3, 2])
        assert q["n_waves"] == [1] and q["wave0"] == [0, 8, 8]
    assert plan(harness, 0, LENS)["n_waves"] == [1]  # width < 1: the default, 256


def test_nothing_to_score_gives_no_waves(harness):
    p = plan(harness, 256, [0, 1, 1, 0])
    assert p["n_rows"] == [0] and p["n_waves"] == [0] and p["order"] == []


def test_refusals_need_no_device():
    """-1 with nothing computed, and 0 for an empty batch, on a machine without a GPU (here no compute entry point
    is reached: with a device present the same calls return before they touch it)."""
    lib = rc.bind_char(rc.load_amd())
    net = lib.rnn_new(42, 39, 42, rc.FLAG_STANDARD, 1, None, 4, 1e-3, 0.9, 0.0, rc.RELU)
    text = np.arange(10, dtype=np.uint8)
    ptrs = (rc.c_u8_p * 1)(rc.u8ptr(text))
    lens = np.array([10], np.int32)
    sums = np.full(8, 7.0)
    out = sums.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.rnn_amd_run_texts_heads(net, ptrs, rc.iptr(lens), None, 1, 5, out) == -1   # 42 is not heads of 5
    assert lib.rnn_amd_run_texts_heads(net, ptrs, rc.iptr(lens), None, 1, 0, out) == -1
    assert lib.rnn_amd_run_texts(net, ptrs, rc.iptr(lens), None, -1, out) == -1
    assert lib.rnn_amd_run_texts(net, None, rc.iptr(lens), None, 1, out) == -1            # a NULL array
    assert lib.rnn_amd_run_texts(net, ptrs, None, None, 1, out) == -1
    assert lib.rnn_amd_run_texts(net, ptrs, rc.iptr(lens), None, 1, None) == -1
    assert lib.rnn_amd_char_cross_entropy_texts(net, None, ptrs, rc.iptr(lens), -1, 0, None, 0, out) == -1
    bottom = lib.rnn_new_with_bottom_layer(42, 16, 39, 42, rc.FLAG_STANDARD, 5, None, 4, 1e-3, 0.9, 0.0, rc.RELU, 0)
    assert lib.rnn_amd_run_texts(bottom, ptrs, rc.iptr(lens), None, 1, out) == -1
    assert lib.rnn_amd_run_texts_heads(bottom, ptrs, rc.iptr(lens), None, 1, 14, out) == -1
    assert np.all(sums == 7.0)                                                             # nothing computed
    assert lib.rnn_amd_run_texts(net, None, None, None, 0, None) == 0                     # an empty batch
    assert lib.rnn_amd_run_texts_heads(net, None, None, None, 0, 14, None) == 0
    # texts with nothing to score are zeros, and nobody asks for a device
    short = np.array([1, 0], np.int32)
    two = (rc.c_u8_p * 2)(rc.u8ptr(text), None)
    assert lib.rnn_amd_run_texts(net, two, rc.iptr(short), None, 2, out) == 0 and list(sums[:2]) == [0.0, 0.0]
    lib.rnn_delete_net(bottom)
    lib.rnn_delete_net(net)
