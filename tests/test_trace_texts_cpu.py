"""rnn_amd_trace_texts (include/recur_amd.h, recur_amd/csrc/texts_api.c) where it needs no device: everything it refuses
returns -1 with nothing written, and a batch with nothing to trace returns 0 with nothing written -- both before any
compute entry point is reached, so this module passes on a machine without a GPU (with a device present the same calls
return before they touch it).  texts_plan.h's offsets of a wave's trace are asked through tests/texts_plan_harness.c's
plan: prefix sums of (len - 1) * heads in plan order.  What the call computes is tests/test_gpu_trace_texts.py's."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import recur_ctypes as rc
from recur_amd.drivers import TRACE_GUARD, trace_texts


@pytest.fixture(scope="module")
def lib():
    return rc.bind_char(rc.load_amd())


def test_refusals_and_empty_calls_need_no_device(lib):
    net = lib.rnn_new(42, 39, 42, rc.FLAG_STANDARD, 1, None, 4, 1e-3, 0.9, 0.0, rc.RELU)
    bottom = lib.rnn_new_with_bottom_layer(42, 16, 39, 42, rc.FLAG_STANDARD, 5, None, 4, 1e-3, 0.9, 0.0, rc.RELU, 0)
    wide = lib.rnn_new(42, 39, 600, rc.FLAG_STANDARD, 1, None, 4, 1e-3, 0.9, 0.0, rc.RELU)
    texts = [np.array([3, 4, 5], np.uint8), np.array([6], np.uint8), np.array([7, 8], np.uint8)]
    ptrs = (rc.c_u8_p * 3)(*[rc.u8ptr(t) for t in texts])
    lens = np.array([3, 1, 2], np.int32)
    logp = [np.full(8, np.nan, np.float32) for _ in texts]
    guess = [np.full(8, 0xEE, np.uint8) for _ in texts]
    lpp = (rc.c_float_p * 3)(*[rc.fptr(a) for a in logp])
    gsp = (rc.c_u8_p * 3)(*[rc.u8ptr(a) for a in guess])

    def call(net=net, texts=ptrs, lens=rc.iptr(lens), n=3, alen=0, logp=lpp, guess=gsp):
        return lib.rnn_amd_trace_texts(net, texts, lens, n, alen, logp, guess)

    def untouched():
        return all(np.all(np.isnan(a)) for a in logp) and all(np.all(a == 0xEE) for a in guess)

    # everything rnn_amd_run_texts_heads refuses (alphabet_len == 0 is no refusal here: one head as wide as the row)
    assert call(net=None) == -1 and call(net=bottom) == -1 and call(n=-1) == -1
    assert call(texts=None) == -1 and call(lens=None) == -1
    assert call(alen=5) == -1 and call(alen=-14) == -1      # 42 outputs are not heads of 5
    assert call(texts=(rc.c_u8_p * 3)(rc.u8ptr(texts[0]), rc.u8ptr(texts[1]), None)) == -1
    # ... and what is refused about the arrays to trace into
    assert call(logp=None) == -1 and call(logp=None, guess=None) == -1
    assert call(logp=(rc.c_float_p * 3)(None, rc.fptr(logp[1]), rc.fptr(logp[2]))) == -1
    assert call(logp=(rc.c_float_p * 3)(rc.fptr(logp[0]), rc.fptr(logp[1]), None), guess=None) == -1
    assert call(guess=(rc.c_u8_p * 3)(rc.u8ptr(guess[0]), rc.u8ptr(guess[1]), None)) == -1
    assert call(net=wide) == -1                             # a guess among 600 outputs does not fit a byte
    assert call(net=wide, alen=300) == -1
    assert untouched()
    # the refusals come first, also where nothing would be traced
    short = np.array([1, 1, 0], np.int32)
    assert call(net=bottom, lens=rc.iptr(short)) == -1 and call(alen=5, lens=rc.iptr(short)) == -1
    assert call(logp=None, lens=rc.iptr(short)) == -1
    # nothing to trace: 0 at once, nothing written, no device asked for
    assert call(n=0, texts=None, lens=None, logp=None, guess=None) == 0
    assert call(n=0) == 0
    assert call(lens=rc.iptr(short)) == 0 and call(lens=rc.iptr(short), guess=None) == 0
    assert call(lens=rc.iptr(short), alen=14) == 0
    # a text shorter than 2 symbols needs no array, nor a text
    none = (rc.c_float_p * 3)(None, None, None)
    assert call(lens=rc.iptr(short), logp=none, guess=(rc.c_u8_p * 3)(None, None, None)) == 0
    assert call(lens=rc.iptr(short), texts=(rc.c_u8_p * 3)(None, None, None), logp=none, guess=None) == 0
    assert untouched()
    # the driver: empty arrays of the right shapes, its guards in place
    got = trace_texts(lib, net, [np.array([3], np.uint8), np.zeros(0, np.uint8)], alphabet_len=14)
    assert [(a.shape, b.shape) for a, b in got] == [((0, 3), (0, 3))] * 2
    got = trace_texts(lib, net, [], guesses=False)
    assert got == [] and TRACE_GUARD >= 1
    with pytest.raises(ValueError):
        trace_texts(lib, bottom, [np.array([3], np.uint8)])
    for x in (net, bottom, wide):
        lib.rnn_delete_net(x)


TRACE_HARNESS = r"""
#include <stdio.h>
#include "texts_plan.h"
int main(int argc, char **argv) {
  int lens[64], n = 0, width = atoi(argv[1]), per_step = atoi(argv[2]);
  for (int k = 3; k < argc; k++) lens[n++] = atoi(argv[k]);
  TextsPlan p;
  if (texts_plan_make(&p, lens, NULL, n, width)) return 1;
  for (int w = 0; w < p.n_waves; w++) {
    unsigned long long off[64];
    const unsigned long long total = texts_plan_trace_offsets(&p, w, per_step, off);
    printf("%llu:", total);
    for (int j = 0; j < p.waves[w].nrows; j++) printf(" %d@%llu", p.order[p.waves[w].row0 + j], off[j]);
    printf("\n");
  }
  texts_plan_free(&p);
  return 0;
}
"""


@pytest.mark.parametrize("compiler,flags", [("gcc", ["-std=gnu11"]), ("g++", ["-std=c++17", "-x", "c++"])])
def test_a_waves_trace_offsets_are_prefix_sums_in_plan_order(tmp_path, compiler, flags):
    """texts_plan.h stays plain C and valid C++ with the offsets in it; wave 0's total is the largest"""
    src = tmp_path / "trace_offsets.c"
    src.write_text(TRACE_HARNESS)
    exe = str(tmp_path / "trace_offsets")
    subprocess.run([compiler, "-O1", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", rc.ROOT + "/recur_amd/csrc", str(src), "-o", exe], check=True)
    lens = [5, 1, 9, 2, 0, 9, 3, 4]
    for width, heads in ((256, 1), (3, 1), (3, 50), (1, 2)):
        out = subprocess.run([exe, str(width), str(heads)] + [str(n) for n in lens], capture_output=True, text=True,
                             check=True).stdout.splitlines()
        rows = sorted((k for k, n in enumerate(lens) if n >= 2), key=lambda k: (-lens[k], k))
        waves = [rows[a:a + width] for a in range(0, len(rows), width)]
        assert len(out) == len(waves)
        totals = []
        for line, wave in zip(out, waves):
            total, _, rest = line.partition(":")
            at, want = 0, []
            for k in wave:
                want.append("%d@%d" % (k, at))
                at += (lens[k] - 1) * heads
            assert rest.split() == want and int(total) == at
            totals.append(at)
        assert totals[0] == max(totals)
