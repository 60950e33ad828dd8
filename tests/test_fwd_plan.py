"""Which kernels a forward pass (ramd_launch_forward) gets, asked of the rule itself (recur_amd/csrc/fwd_plan.h) without a
GPU: fwd_plan_harness.cpp is compiled with the host compiler alone and prints the plan for a shape, the call's description
and the switches in its environment.  The expected values are worked out by hand from the conditions the launchers and
set_forward had before the plan was split from them; I is 1 + input + hidden rounded up to 4, H is hidden + 1 rounded up
to 4, O is output rounded up to 4.

pick_ks (k_tiles.h) by hand: cost(k) = p * nkt / k + 2 * max(1, p / 3) + 0.15 k with p = ceil(tiles * k / 256), the first
smallest over k = 1 .. min(16, nkt); then as many planes as fit the workspace."""
import os
import subprocess

import pytest

import recur_ctypes as rc

ROOT = rc.ROOT
CSRC = os.path.join(ROOT, "recur_amd", "csrc")
KEEP, ONE_HOT, DENSE, TEXT = 0, 1, 2, 3   # RAMD_IN_*
WHOLE, TEXT_TOP, DENSE_TOP = 0, 1, 2      # RAMD_FWD_*
SRC = os.path.join(ROOT, "tests", "fwd_plan_harness.cpp")
CXX = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include")]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fwd_plan") / "fwd_plan_harness")
    subprocess.run(CXX + [SRC, "-o", exe], check=True)
    return exe


def plan(exe, env=None, **args):
    e = {k: v for k, v in os.environ.items() if not k.startswith("RECUR_AMD_")}
    e.update(env or {})
    out = subprocess.run([exe] + ["%s=%d" % kv for kv in args.items()], env=e, capture_output=True, text=True, check=True).stdout
    d = dict(line.split("=", 1) for line in out.splitlines())
    return {k: int(v) if v.lstrip("-").isdigit() else v for k, v in d.items()}


def has(p, **want):
    got = {k: p.get(k) for k in want}
    assert got == want


def shape(i, h, o, rows, **more):
    return dict(input=i, hidden=h, output=o, streams=rows, **more)


def text_step(i, h, o, rows, **more):  # char_step_deltas: advance, the sums left for ramd_launch_text_top
    return shape(i, h, o, rows, mode=TEXT, advance=1, want=TEXT_TOP, **more)


def fwd_rows(i, h, o, rows, **more):  # rnn_amd_set_opinion on forward-only rows (above Scap; no shared ring position)
    return dict(input=i, hidden=h, output=o, streams=256, nrows=rows, mode=DENSE, advance=0, fwd_only=1, uniform_idx=-1, **more)


BENCH = text_step(42, 1024, 42, 256)
MULTI = shape(75, 1024, 3650, 256, mode=ONE_HOT, advance=1)  # the multi-head step's pass: I = 1100, H = 1028, O = 3652
# tiles 4 x 17 = 68, nkt = ceil(1068 / 32) = 34: p = 1 up to k = 3 (204 workgroups), 2 up to 7, 3 up to 11, 4 up to 15;
# the best of each p: k = 3: 11.33 + 2 + 0.45 = 13.78; k = 7: 2 * 4.857 + 2 + 1.05 = 12.76; k = 11: 3 * 3.09 + 2 + 1.65 =
# 12.92; k = 15: 4 * 2.267 + 2.67 + 2.25 = 13.98; k = 16 (p = 5): 16.36 -> 7
BENCH_KS = 7


def test_the_header_needs_no_hip():
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-x", "c++",
                    os.path.join(CSRC, "fwd_plan.h")], check=True)


def test_the_text_step_fused(harness):
    # tm = 256 / 32 = 8, tn = 1024 / 32 = 32, blocks = ceil(32 / 8) * 8 * 8 = 256; 1024 / 128 = 8 whole stages
    has(plan(harness, **BENCH), I=1068, H=1028, O=44, input="inside", hidden="fused", ns=8, nstages=8, tm=8, tn=32, blocks=256,
        noise="none", end="left", left_planes=1, left_partials=32, output="none")
    # tm = 4, tn = 16, blocks = 2 * 8 * 4 = 64; 512 / 128 = 4 stages
    has(plan(harness, **text_step(42, 512, 42, 128)), hidden="fused", ns=4, nstages=4, tm=4, tn=16, blocks=64, left_partials=16)
    # 704 = 5.5 x 128: six stages, the last partial -> the form for any number; tn = 22, blocks = 3 * 8 * 1 = 24
    has(plan(harness, **text_step(42, 704, 42, 32)), hidden="fused", ns=0, nstages=6, tm=1, tn=22, blocks=24, left_partials=22)
    # 96 = 0.75 x 128: one partial stage; 2048 = 16 stages
    has(plan(harness, **text_step(42, 96, 42, 32)), hidden="fused", ns=0, nstages=1, tn=3, blocks=8)
    has(plan(harness, **text_step(42, 2048, 42, 32)), hidden="fused", ns=16, nstages=16, tm=1, tn=64, blocks=64)


def test_the_text_step_where_the_fused_launch_declines(harness):
    generic = dict(input="assemble", hidden="gemm", nkt=34, ks=BENCH_KS, end="left", left_planes=BENCH_KS, left_partials=0,
                   output="none")
    has(plan(harness, {"RECUR_AMD_NO_FWD_FUSED": "1"}, **BENCH), uniform=1, noise="none", **generic)
    # presynaptic noise: the top launch takes the sums as the forward pass leaves them, and the fused launch adds none
    has(plan(harness, **BENCH, noise=1), uniform=1, noise="generate", **generic)
    has(plan(harness, **BENCH, noise=1, noise_spec_use=1), uniform=1, noise="apply", **generic)
    has(plan(harness, **BENCH, uniform_idx=-1), uniform=0, noise="none", **generic)
    # 99 is not a multiple of 32.  I = 144, H = 100: tiles 1 x 2, nkt = 5, p = 1: 5 / k + 2 + 0.15 k falls to k = 5 (3.75)
    has(plan(harness, **text_step(42, 99, 42, 1)), input="assemble", hidden="gemm", nkt=5, ks=5, left_planes=5)
    # the plan asks ramd_text_top_ok's question itself ...
    has(plan(harness, {"RECUR_AMD_NO_TEXT_TOP": "1"}, **BENCH), input="assemble", hidden="gemm")
    # ... and callers that asked it up front want the whole pass: fused, its own finishing kernel, k_out_layer (O = 44)
    has(plan(harness, {"RECUR_AMD_NO_TEXT_TOP": "1"}, **dict(BENCH, want=WHOLE)), input="inside", hidden="fused", ns=8,
        end="finalize_fused", tn=32, noise="none", output="rows", left_planes=0, left_partials=0)


def test_the_workspace_must_hold_sums_and_partials(harness):
    need = 256 * 1028 + 32 * 256 * 4  # plane 0 + [tn][nrows][4]
    has(plan(harness, **BENCH, slab_floats=need), hidden="fused")
    # one float less: the GEMM, and of its 7 planes of 256 * 1028 only one fits
    has(plan(harness, **BENCH, slab_floats=need - 1), input="assemble", hidden="gemm", ks=1, left_planes=1, left_partials=0)


def test_the_multi_head_pass(harness):
    # output: H = 1028 is 17 stages of 64; 256 / 64 = 4 row tiles x ceil(3652 / 64) = 58 column tiles = 232 >= 128;
    # supertiles ceil(4 / 4) * ceil(58 / 8) = 8 -> 8 * 32 = 256 workgroups
    wide_out = dict(output="wide", o_ns=17, o_tm=4, o_tn=58, o_blocks=256)
    has(plan(harness, **MULTI, noise=1, noise_spec_use=1), I=1100, O=3652, input="inside", hidden="fused", ns=8, tm=8, tn=32,
        noise="apply", end="finalize_fused", **wide_out)
    has(plan(harness, **MULTI), hidden="fused", noise="none", end="finalize_fused", **wide_out)
    # noise that was not generated ahead: k_presynaptic_noise needs the GEMM's plane.  nkt = ceil(1100 / 32) = 35, tiles 68:
    # k = 7: 2 * 5 + 2 + 1.05 = 13.05; k = 11: 3 * 3.18 + 2 + 1.65 = 13.2; k = 3: 11.67 + 2.45 = 14.1 -> 7
    has(plan(harness, **MULTI, noise=1), input="assemble", hidden="gemm", uniform=1, nkt=35, ks=7, noise="generate",
        end="finalize", **wide_out)
    # o_nkt = ceil(1028 / 32) = 33, tiles 4 x 58 = 232: k = 1: 33 + 2 + 0.15 = 35.15; k = 2 (p = 2): 33 + 2 + 0.3; k = 3 (p = 3):
    # 33 + 2 + 0.45; from k = 4 on p > 3 and the fill charge grows -> 1
    has(plan(harness, {"RECUR_AMD_OUT_WIDE": "0"}, **MULTI, noise=1, noise_spec_use=1), hidden="fused", output="gemm", o_nkt=33, o_ks=1)
    has(plan(harness, {"RECUR_AMD_FWD_FUSED_ANY": "0"}, **MULTI, noise=1, noise_spec_use=1), input="assemble", hidden="gemm",
        ks=7, noise="apply", end="finalize", **wide_out)
    # without advancing (rnn_amd_set_one_hot_opinion) the ring slot is the old one: never fused
    has(plan(harness, **dict(MULTI, advance=0)), input="assemble", hidden="gemm")


def test_a_wide_output_layer_on_a_narrow_hidden_layer(harness):
    # H = 100: ceil(100 / 64) = 2 stages, not 9 / 17 / 33.  Hidden: I = 176, tiles 1 x 2, nkt = 6: 6 / k + 2 + 0.15 k falls to
    # k = 6 (3.9).  Output: tiles ceil(rows / 64) x 58, o_nkt = ceil(100 / 32) = 4, p = 1: 4 / k + 2 + 0.15 k falls to k = 4 (3.6)
    narrow = shape(75, 99, 3650, 32, mode=ONE_HOT, advance=1)
    has(plan(harness, **narrow), input="assemble", hidden="gemm", nkt=6, ks=6, end="finalize", output="gemm", o_nkt=4, o_ks=4)
    # (at 256 rows, a multiple of 64 with 232 tiles, only the stage count declines: p = 1 up to k = 1, so
    # k = 1: 4 + 2.15 = 6.15; k = 2 (p = 2): 4 + 2.3; k = 3 (p = 3): 4 + 2.45; k = 4 (p = 4): 4 + 2.67 + 0.6 -> 1)
    has(plan(harness, **dict(narrow, streams=256)), output="gemm", o_ks=1)
    # the smallest wide output layer: H = 516 is 9 stages, 2 x 64 = 128 tiles; supertiles 1 * 8 -> 256 workgroups
    has(plan(harness, **shape(42, 512, 4096, 128, mode=ONE_HOT, advance=1)), output="wide", o_ns=9, o_tm=2, o_tn=64, o_blocks=256)
    has(plan(harness, **shape(42, 512, 4032, 128, mode=ONE_HOT, advance=1)), output="gemm")  # 2 x 63 = 126 tiles


def test_dense_inputs_for_the_dense_top(harness):
    dense_top = dict(mode=DENSE, advance=0, want=DENSE_TOP)
    # tm = 2, tn = 16: 32 tiles, blocks = 2 * 8 * 2 = 32; gstclassify's 512 / 128: 4 x 16 = 64
    has(plan(harness, **shape(35, 512, 3, 64, **dense_top)), input="inside", hidden="fused", ns=4, tm=2, tn=16, blocks=32,
        end="left", left_planes=1, left_partials=16, output="none")
    has(plan(harness, **shape(35, 512, 3, 128, **dense_top)), hidden="fused", tm=4, tn=16, blocks=64)
    # 16 x 64 = 1024 tiles > 256.  I = 2084, H = 2052: tiles 8 x 33 = 264, nkt = ceil(2084 / 32) = 66, p = k + 1:
    # k = 8: 9 * 8.25 + 6 + 1.2 = 81.45; k = 9: 10 * 7.333 + 6.667 + 1.35 = 81.35; k = 10: 11 * 6.6 + 7.333 + 1.5 = 81.43 -> 9
    has(plan(harness, **shape(35, 2048, 3, 512, **dense_top)), input="assemble", hidden="gemm", uniform=1, nkt=66, ks=9,
        end="left", left_planes=9, left_partials=0)
    has(plan(harness, **shape(35, 1024, 3, 256, **dense_top)), hidden="fused", tm=8, tn=32)  # exactly 256 tiles
    # 100 inputs > FF_MAXIN = 64.  I = 1128, tiles 1 x 17, nkt = 36, p = 1 up to k = 15: 36 / k + 2 + 0.15 k: k = 14: 6.67,
    # k = 15: 6.65; k = 16 (p = 2): 8.9 -> 15
    has(plan(harness, **shape(100, 1024, 10, 32, **dense_top)), input="assemble", hidden="gemm", ks=15, left_planes=15)
    # I = 548, H = 516: tiles 1 x 9, nkt = 18, p = 1: 18 / k + 2 + 0.15 k: k = 10: 5.3, k = 11: 5.286, k = 12: 5.3 -> 11
    has(plan(harness, {"RECUR_AMD_FWD_FUSED_DENSE": "0"}, **shape(35, 512, 3, 64, **dense_top)), input="assemble", hidden="gemm",
        nkt=18, ks=11)
    has(plan(harness, **shape(35, 512, 3, 64, **dict(dense_top, dense=0))), hidden="gemm")  # no inputs on the device
    # the same inputs through rnn_amd_set_opinion: the whole pass; O = 4 and 64 rows: k_out_layer_o4; fewer rows: k_out_layer
    has(plan(harness, **shape(35, 512, 3, 64, mode=DENSE, advance=0)), hidden="fused", end="finalize_fused", output="o4")
    has(plan(harness, **shape(35, 512, 3, 32, mode=DENSE, advance=0)), hidden="fused", end="finalize_fused", output="rows")


def test_forward_only_rows(harness):
    # I = 2092: ceil(2092 / 64) = 33 stages; 13824 / 64 = 216 row tiles, ceil(2052 / 64) = 33 column tiles;
    # supertiles ceil(216 / 4) * ceil(33 / 8) = 54 * 5 = 270 -> ceil(270 / 8) * 8 * 32 = 8704 workgroups
    has(plan(harness, **fwd_rows(42, 2048, 3, 13824)), input="assemble", hidden="wide", ns=33, tm=216, tn=33, blocks=8704, ks=1,
        end="finalize", output="o4")
    # I = 556: 9 stages; 32 x ceil(516 / 64) = 9 tiles; supertiles 8 * 2 = 16 -> 512 workgroups
    has(plan(harness, **fwd_rows(42, 512, 42, 2048)), hidden="wide", ns=9, tm=32, tn=9, blocks=512, output="rows")
    has(plan(harness, {"RECUR_AMD_FWD_WIDE": "0"}, **fwd_rows(42, 512, 42, 2048)), hidden="gemm", uniform=0)
    has(plan(harness, **fwd_rows(42, 512, 42, 2047)), hidden="gemm", uniform=0)  # not a multiple of 64
    has(plan(harness, **fwd_rows(42, 512, 42, 1984)), hidden="gemm")             # 31 x 64, below 2048
    has(plan(harness, **fwd_rows(42, 256, 42, 2048)), hidden="gemm")             # I = 300: 5 stages
    # the plane of sums must fit the workspace (here 2048 * 516 floats)
    has(plan(harness, **fwd_rows(42, 512, 42, 2048), slab_floats=2048 * 516), hidden="wide")
    # the batched text scorer's rows come built
    has(plan(harness, **dict(fwd_rows(42, 512, 42, 2048), mode=KEEP, rows_built=1)), input="built", hidden="wide")
    has(plan(harness, **dict(fwd_rows(42, 512, 42, 100), mode=KEEP, rows_built=1)), input="built", hidden="gemm", end="finalize",
        output="rows")


@pytest.mark.parametrize("call", [BENCH, dict(BENCH, want=WHOLE), dict(MULTI, noise=1, noise_spec_use=1),
                                  shape(35, 512, 3, 64, mode=DENSE, advance=0, want=DENSE_TOP),
                                  shape(42, 99, 42, 1, mode=KEEP, advance=0, one_net=1),
                                  shape(42, 99, 42, 1, mode=TEXT, advance=0)])
def test_a_bottom_layer(harness, call):
    p = plan(harness, **call, bottom=20)
    has(p, input="bottom", advance_first=call["advance"])
    assert p["hidden"] in ("gemm", "wide")
    assert p["noise"] == ("apply" if call.get("noise_spec_use") else "generate" if call.get("noise") else "none")
    has(plan(harness, **call), advance_first=0)


def test_one_net(harness):
    small = shape(42, 99, 42, 1, mode=KEEP, advance=0, one_net=1)
    has(plan(harness, **small), input="inside", hidden="small", end="inside", output="inside", noise="none")
    # I = 144, H = 100: nkt = 5, ks = 5 (as in the text step above)
    generic = dict(input="assemble", hidden="gemm", nkt=5, ks=5, end="finalize", output="rows")
    has(plan(harness, **small, noise=1), noise="generate", **generic)
    has(plan(harness, {"RECUR_AMD_FWD_SMALL": "0"}, **small), noise="none", **generic)
    has(plan(harness, **dict(small, one_net=0)), **generic)  # the per-net text loop never asked for the small form
    # H = 304 > 256.  I = 344: tiles 1 x 5, nkt = 11, p = 1: 11 / k + 2 + 0.15 k: k = 8: 4.575, k = 9: 4.572, k = 10: 4.6 -> 9
    has(plan(harness, **dict(small, hidden=300)), input="assemble", hidden="gemm", nkt=11, ks=9, end="finalize", output="rows")
    has(plan(harness, **dict(small, hidden=252)), hidden="small")  # H = 256, I = 296
    has(plan(harness, **dict(small, hidden=252, input=260)), hidden="gemm")  # I = 516 > 512
    has(plan(harness, **dict(small, output=65)), hidden="gemm")  # O = 68 > 64


def test_the_batched_text_runs_shrinking_passes(harness):
    """rnn_amd_run_texts and rnn_amd_sample_texts: built rows above Scap, no ring position, a row count that falls from
    the wave's 256 to 1 as texts end.  The shapes are those of tests/test_gpu_texts_wide.py: if a predicate moves, this
    says which form its nets no longer reach."""
    def texts(i, h, o, rows):
        return dict(input=i, hidden=h, output=o, streams=256, nrows=rows, mode=KEEP, rows_built=1, fwd_only=1, advance=0,
                    uniform_idx=-1)

    # A 42 / 1024 / 42: I = 1068, H = 1028, O = 44; nkt = 34, column tiles ceil(1028 / 64) = 17.  256 rows: 68 tiles, BENCH_KS.
    # 192: 51 tiles, p = 1 up to k = 5 (255), 2 up to 10, 3 up to 15: k = 5: 6.8 + 2 + 0.75 = 9.55; k = 10: 2 * 3.4 + 2 + 1.5 =
    # 10.3; k = 15: 3 * 2.267 + 2 + 2.25 = 11.05; k = 16 (p = 4): 4 * 2.125 + 2.67 + 2.4 = 13.57 -> 5
    # 128 and 65: 34 tiles, p = 1 up to k = 7 (238), 2 up to 15: k = 7: 4.857 + 2 + 1.05 = 7.91; k = 15: 2 * 2.267 + 2 + 2.25 =
    # 8.78; k = 16 (p = 3): 3 * 2.125 + 2 + 2.4 = 10.78 -> 7
    # 64 and fewer: 17 tiles, p = 1 up to k = 15 (255): k = 14: 2.429 + 2 + 2.1 = 6.529; k = 15: 2.267 + 2 + 2.25 = 6.517;
    # k = 16 (p = 2): 2 * 2.125 + 2 + 2.4 = 8.65 -> 15
    for rows, ks in [(256, BENCH_KS), (192, 5), (128, 7), (65, 7), (64, 15), (63, 15), (17, 15), (1, 15)]:
        has(plan(harness, **texts(42, 1024, 42, rows)), I=1068, H=1028, O=44, input="built", hidden="gemm", uniform=0, nkt=34,
            ks=ks, noise="none", end="finalize", output="rows")
    # B 73 / 99 / 3650 (the multi-head text net): I = 176, H = 100, O = 3652.  Hidden: nkt = 6, at most 4 x 2 tiles, p = 1:
    # 6 / k + 2 + 0.15 k falls to k = 6 (3.9).  Output: o_nkt = 4, column tiles ceil(3652 / 64) = 58.  256 and 200 rows: 232
    # tiles -> 1 (test_a_wide_output_layer_on_a_narrow_hidden_layer).  128: 116 tiles: k = 1: 4 + 2 + 0.15 = 6.15; k = 2 (232,
    # p = 1): 2 + 2 + 0.3 = 4.3; k = 3 (p = 2): 2 * 1.333 + 2 + 0.45 = 5.12; k = 4 (p = 2): 2 + 2 + 0.6 = 4.6 -> 2.  64 and
    # fewer: 58 tiles, p = 1 up to k = 4 (232): 4 / k + 2 + 0.15 k: k = 3: 3.78; k = 4: 3.6 -> 4
    for rows, o_ks in [(256, 1), (200, 1), (128, 2), (64, 4), (63, 4), (5, 4), (1, 4)]:
        has(plan(harness, **texts(73, 99, 3650, rows)), I=176, H=100, O=3652, input="built", hidden="gemm", nkt=6, ks=6,
            end="finalize", output="gemm", o_nkt=4, o_ks=o_ks)
    # C 128 / 512 / 4096: I = 644, H = 516 (9 stages of 64), O = 4096 (64 column tiles).  Output: 4, 3 and 2 row tiles x 64 >=
    # 128 tiles, supertiles ceil(tm / 4) * 8 = 8 -> 256 workgroups.  Hidden: nkt = ceil(644 / 32) = 21, column tiles 9.
    # 256 rows: 36 tiles, p = 1 up to k = 7 (252), 2 up to 14: k = 7: 3 + 2 + 1.05 = 6.05; k = 14: 2 * 1.5 + 2 + 2.1 = 7.1 -> 7
    # 192: 27 tiles, p = 1 up to k = 9 (243), 2 up to 16: k = 9: 2.333 + 2 + 1.35 = 5.68; k = 16: 2 * 1.3125 + 2 + 2.4 = 7.03 -> 9
    # 128: 18 tiles, p = 1 up to k = 14 (252): 21 / k + 0.15 k: k = 11: 3.559; k = 12: 3.55; k = 13: 3.565 -> 12
    for rows, tm, ks in [(256, 4, 7), (192, 3, 9), (128, 2, 12)]:
        has(plan(harness, **texts(128, 512, 4096, rows)), I=644, H=516, O=4096, input="built", hidden="gemm", nkt=21, ks=ks,
            end="finalize", output="wide", o_ns=9, o_tm=tm, o_tn=64, o_blocks=256)
    # 64 rows are 64 tiles, fewer than 128; 1 row is no multiple of 64.  o_nkt = ceil(516 / 32) = 17, 64 tiles: p = 1 up to
    # k = 4 (256), 2 up to 8, 3 up to 12: k = 4: 4.25 + 2 + 0.6 = 6.85; k = 8: 2 * 2.125 + 2 + 1.2 = 7.45; k = 12: 3 * 1.417 + 2 +
    # 1.8 = 8.05; k = 16 (p = 4): 4 * 1.0625 + 2.67 + 2.4 = 9.32 -> 4
    for rows in (64, 1):
        has(plan(harness, **texts(128, 512, 4096, rows)), input="built", hidden="gemm", nkt=21, output="gemm", o_nkt=17, o_ks=4)
    # D 4 / 64 / 4: I = 72, H = 68, O = 4.  nkt = 3, at most 2 tiles, p = 1: 3 / k + 2 + 0.15 k falls to k = 3 (3.45)
    has(plan(harness, **texts(4, 64, 4, 64)), I=72, H=68, O=4, input="built", hidden="gemm", nkt=3, ks=3, end="finalize", output="o4")
    has(plan(harness, **texts(4, 64, 4, 63)), input="built", hidden="gemm", nkt=3, ks=3, end="finalize", output="rows")
