"""The cases of tests/test_gpu_staggered_rings.py (a training set whose streams sit at DIFFERENT positions of their BPTT
rings, so that every plan declines its lock-step form) and what tests/test_staggered_rings_cpu.py proves about them
without a GPU: which kernels each case gets, and that its stagger would notice a wrong row rule.

The stagger: before the first step stream j is advanced `extra_advances(j, D)` times more than stream 0's neighbours --
(3 j + 1) % D, which visits every ring position where 3 does not divide D.  Where it does (D = 6, 9, 12) that formula
only ever lands on D / 3 positions, so one more step is added after every D / 3 streams; the sets then hold min(D, S)
distinct positions for every depth, which is what the GPU tests assert in front of the generation they compare."""
import math

import numpy as np

import recur_ctypes as rc


def extra_advances(j, D):
    period = D // math.gcd(3, D)
    return (3 * j + 1 + (j // period if period < D else 0)) % D


def stagger_offsets(S, D):
    return np.array([extra_advances(j, D) for j in range(S)], np.int32)


def stagger_device(g):
    """rnn_bptt_advance on the clones of a device set (the host's index is the authority: net_api.c, ramd_push_indices)"""
    for j in range(g.S):
        for _ in range(extra_advances(j, g.D)):
            g.lib.rnn_bptt_advance(g.nets[j])


def stagger_oracle(o):
    for j in range(o.S):
        for _ in range(extra_advances(j, o.D)):
            o.orc.orc_advance(o.z, j)


def distinct_positions(index):
    return len(set(int(x) for x in index))


# ---------------------------------------------------------------- the row rule, restated --
# k_common.h, input_row<false>: the history row of stream r, `back` steps ago, is slot idx[r] - back of its ring, plus D
# where that is negative.  The mutants are the mistakes a kernel could make and still pass every lock-step test.

def slot_rule(idx, back, D):
    slot = idx - back
    return np.where(slot < 0, slot + D, slot)


def slot_first_row_for_all(idx, back, D):      # the tile's first row speaks for every row (the <true> form's shortcut)
    return slot_rule(np.full_like(idx, idx[0]), back, D)


def slot_without_the_wrap(idx, back, D):
    return idx - back


def slot_wrapped_one_short(idx, back, D):
    slot = idx - back
    return np.where(slot < 0, slot + D - 1, slot)


MUTANTS = {"first_row_for_all": slot_first_row_for_all, "without_the_wrap": slot_without_the_wrap,
           "wrapped_one_short": slot_wrapped_one_short}


def first_difference(mutant, S, D, generations):
    """(stream, step back) at which the mutant first picks another row than the rule, for a set of S streams staggered as
    above and then advanced `generations` times together; None if it never does"""
    idx = (stagger_offsets(S, D) + generations) % D
    for back in range(D):
        differs = np.nonzero(mutant(idx, back, D) != slot_rule(idx, back, D))[0]
        if len(differs):
            return int(differs[0]), back
    return None


# ---------------------------------------------------------------------------- the cases --
# kw: what the set is made with (input 42 / output 42 / RELU unless the case is about something else); steps: how the
# case is driven -- "text" (rnn_amd_set_char_step), "multi" (the multi-head step), "dense" (gstclassify's order with an
# active mask), "bottom" (the same on a bottom layer).
# chain / calc / fwd: what chain_plan.h, calc_plan.h and fwd_plan.h give the call with uniform_idx = -1, worked out by hand:
#   I = 1 + input + hidden rounded up to 4, H = hidden + 1 rounded up to 4, O = output rounded up to 4
#   chain: k_chain_main<false, 0>: nstages = ceil(hidden / 128), tm = ceil(S / 32), tn = ceil(hidden / 32), blocks = ceil(tn / 8) 8 tm
#   calc:  nkt = D ceil(S / 32); big = I >= 256 and nkt >= 16: tiles of 128 x 128 over I x hidden, else of 64 x 64;
#          ks = pick_ks(tiles, nkt): the first smallest p nkt / k + 2 max(1, p / 3) + 0.15 k, p = ceil(tiles k / 256), k <= min(16, nkt)
#   fwd:   nkt = ceil(I / 32), tiles = ceil(S / 64) ceil(H / 64), ks by the same rule

def _case(kw, steps, chain, calc, fwd, calc_args=None, fwd_args=None, **more):
    return dict(kw=kw, steps=steps, chain=chain, calc=calc, fwd=fwd, calc_args=calc_args or {}, fwd_args=fwd_args or {}, **more)


def _kw(hidden, S, D, **more):
    return dict(dict(input_size=42, hidden_size=hidden, output_size=42, S=S, D=D), **more)


TEXT_CALC = dict(flags=0x40000000)   # RAMD_TOP_DONE: ramd_launch_text_top has done the top backprop; defer: the update rides along
TEXT_FWD = dict(mode=3, advance=1, want=1)

CASES = {
    # I = 244, H = 204.  calc: nkt = 7 x 3 = 21, 4 x 4 = 16 small tiles (p = 1): 21 / k + 0.15 k: k = 11: 3.559, 12: 3.55, 13: 3.565
    # fwd: nkt = 8, 2 x 4 = 8 tiles: 8 / k + 0.15 k: k = 6: 2.233, 7: 2.193, 8: 2.2
    "tiles_200_70_7": _case(
        _kw(200, 70, 7), "text",
        dict(nstages=2, tm=3, tn=7, blocks=24),
        dict(I=244, H=204, ho_asked=1, big=0, ks=12, top="done", ho_gemm="planes", extras="control5"),
        dict(ks=7, nkt=8, input="assemble", end="left", left_planes=7, left_partials=0, output="none")),
    # I = 108, H = 68.  calc: nkt = 9 x 2 = 18, 2 x 1 tiles: 18 / k + 0.15 k: k = 10: 3.3, 11: 3.286, 12: 3.3
    # fwd: nkt = 4, 1 x 2 tiles: 4 / k + 0.15 k falls to k = 4 (1.6)
    "depth_wrap_64_33_9": _case(
        _kw(64, 33, 9), "text",
        dict(nstages=1, tm=2, tn=2, blocks=16),
        dict(I=108, H=68, ho_asked=1, big=0, ks=11, top="done", ho_gemm="planes", extras="control5"),
        dict(ks=4, nkt=4, input="assemble", end="left", left_planes=4, left_partials=0, output="none")),
    # I = 300, H = 260.  calc: nkt = 5 x 2 = 10 (< 16: small tiles), 5 x 4 = 20 tiles (p = 1 up to k = 12):
    # 10 / k + 0.15 k: k = 7: 2.479, 8: 2.45, 9: 2.461.  fwd: nkt = 10, 1 x 5 tiles: the same sum -> 8
    "resqrt_256_48_5": _case(
        _kw(256, 48, 5, activation=rc.RESQRT), "text",
        dict(nstages=2, tm=2, tn=8, blocks=16),
        dict(I=300, H=260, ho_asked=1, big=0, ks=8, top="done", ho_gemm="planes", extras="control5"),
        dict(ks=8, nkt=10, input="assemble", end="left", left_planes=8, left_partials=0, output="none"),
        calc_args=dict(activation=rc.RESQRT)),
    # I = 176, H = 132.  calc: nkt = 6 x 2 = 12, 3 x 3 = 9 tiles: 12 / k + 0.15 k: k = 8: 2.7, 9: 2.683, 10: 2.7
    # fwd: nkt = 6, 1 x 3 tiles: 6 / k + 0.15 k falls to k = 6 (1.9)
    "reclip20_130_40_6": _case(
        _kw(130, 40, 6, activation=rc.RECLIP20, variance=0.1), "text",
        dict(nstages=2, tm=2, tn=5, blocks=16),
        dict(I=176, H=132, ho_asked=1, big=0, ks=9, top="done", ho_gemm="planes", extras="control5"),
        dict(ks=6, nkt=6, input="assemble", end="left", left_planes=6, left_partials=0, output="none"),
        calc_args=dict(activation=rc.RECLIP20),
        # (the reference's own spread with units at the ceiling: profiles/r08_reference_elementwise_self_difference_reclip20.txt)
        elem_floor=1e-1),
    # I = 796, H = 516.  calc: nkt = 6 x 4 = 24: big, 7 x 4 = 28 tiles of 128 x 128, p = 1 up to k = 9 (252), 2 from 10:
    # k = 8: 3 + 2 + 1.2 = 6.2; k = 9: 2.667 + 2 + 1.35 = 6.017; k = 16 (p = 2): 3 + 2 + 2.4 = 7.4
    # fwd: nkt = 25, 2 x 9 = 18 tiles, p = 1 up to k = 14: 25 / k + 0.15 k: k = 12: 3.883, 13: 3.873, 14: 3.886
    "big_gemm_512_128_6_i280": _case(
        _kw(512, 128, 6, input_size=280), "text",
        dict(nstages=4, tm=4, tn=16, blocks=64),
        dict(I=796, H=516, ho_asked=1, big=1, ks=9, top="done", ho_gemm="planes", extras="control5"),
        dict(ks=13, nkt=25, input="assemble", end="left", left_planes=13, left_partials=0, output="none")),
    # I = 1068, H = 1028.  calc: nkt = 10 x 2 = 20: big, 9 x 8 = 72 tiles, p = 1 up to k = 3, 2 up to 7, 3 up to 10, 4 up to 14:
    # k = 3: 6.667 + 2 + 0.45 = 9.117; k = 7: 2 x 2.857 + 2 + 1.05 = 8.764; k = 10: 3 x 2 + 2 + 1.5 = 9.5; k = 14: 4 x 1.429 + 2.667 + 2.1
    # fwd: nkt = 34, 1 x 17 tiles: 15 (test_fwd_plan.py: test_the_batched_text_runs_shrinking_passes)
    "north_star_width_1024_64_10": _case(
        _kw(1024, 64, 10), "text",
        dict(nstages=8, tm=2, tn=32, blocks=64),
        dict(I=1068, H=1028, ho_asked=1, big=1, ks=7, top="done", ho_gemm="planes", extras="control5"),
        dict(ks=15, nkt=34, input="assemble", end="left", left_planes=15, left_partials=0, output="none")),
    # O = 300 > 256: no text top (the whole pass, the stand-alone softmax, TOP_PLAIN) and, O > 48, nobody is asked for the
    # top layer's delta: its own GEMM, as planes for the update the step's caller has announced (HO_PLANES; without
    # that announcement, HO_SUMMED).  calc: nkt = 5 x 2 = 10, 2 x 1 tiles -> 8 as above.  fwd: nkt = 4 -> 4;
    # output: o_nkt = ceil(68 / 32) = 3, 1 x 5 tiles: 3 / k + 0.15 k falls to k = 3
    "wide_top_64_36_5_o300": _case(
        _kw(64, 36, 5, output_size=300), "text",
        dict(nstages=1, tm=2, tn=2, blocks=16),
        dict(I=108, H=68, O=300, ho_asked=0, big=0, ks=8, top="plain", ho_gemm="planes", extras="control5"),
        dict(ks=4, nkt=4, input="assemble", end="finalize", output="gemm", o_nkt=3, o_ks=3),
        calc_args=dict(flags=0), fwd_args=dict(want=0)),
    # 5 heads of 10 symbols on 40 hidden units, 6 streams: I = 52, H = 44, O = 52.  Heads narrower than 24 columns are plain
    # per-stream ranges (set_loss.c: multi_calc_deltas): the ranged top backprop with min(16, 256 / 6) partial sums per
    # stream and, ranges given, the top layer's own summed GEMM.  No update is announced: the planes go to the set's own
    # workspace (8 I H + 64 x 128 H floats).  calc: nkt = 6, one tile: 6 / k + 0.15 k falls to k = 6.  fwd: nkt = 2 -> 2
    "multi_head": _case(
        dict(input_size=10, hidden_size=40, output_size=50, S=6, D=6, activation=rc.RESQRT), "multi",
        dict(nstages=1, tm=1, tn=2, blocks=8),
        dict(I=52, H=44, O=52, ho_asked=0, big=0, ks=6, top="ranged", top_nb=16, ho_gemm="summed", extras="control5", own_ws=1),
        dict(ks=2, nkt=2, input="assemble", end="finalize", output="rows"),
        calc_args=dict(activation=rc.RESQRT, flags=0, ranges=1, range_stride=132, mheads_alen=10, fuse_want=0,
                       own_slab_floats=8 * 52 * 44 + 64 * 128 * 44),
        fwd_args=dict(mode=1, want=0)),
    # ... and heads wide enough for the per-head kernels, which the shape above does not reach: 56 heads of 35 symbols (the
    # last shape of test_multi_head_generation_matches_oracle), 11 streams, depth 7: I = 76, H = 44, O = 1960.  The sparse
    # top backprop over the partial products (11 x 56 x 44 floats) and k_ho_delta_heads.  calc: nkt = 7, 2 x 1 tiles:
    # 7 / k + 0.15 k: k = 6: 2.067, 7: 2.05.  fwd: nkt = 3 -> 3; output: o_nkt = 2, 1 x 31 tiles: k = 1: 4.15, 2: 3.3
    "multi_head_wide": _case(
        dict(input_size=35, hidden_size=40, output_size=35 * 56, S=11, D=7, activation=rc.RESQRT), "multi",
        dict(nstages=1, tm=1, tn=2, blocks=8),
        dict(I=76, H=44, O=1960, ho_asked=0, big=0, ks=7, top="sparse", ho_gemm="heads", extras="control5", own_ws=1),
        dict(ks=3, nkt=3, input="assemble", end="finalize", output="gemm", o_nkt=2, o_ks=2),
        calc_args=dict(activation=rc.RESQRT, flags=0x10000000, ranges=1, range_stride=132, mheads_alen=35, fuse_want=0,
                       mheads_part_floats=11 * 56 * 44, own_slab_floats=8 * 76 * 44 + 64 * 128 * 44),
        fwd_args=dict(mode=1, want=0)),
    # gstclassify's shape with 33 streams (two row tiles of 32): I = 548, H = 516, O = 4; 36 dense columns: the chain is asked
    # for the dense extras and, declining, leaves them to k_extras_dense.  calc: nkt = 12 x 2 = 24: big, 5 x 4 = 20 tiles,
    # p = 1 up to k = 12: 24 / k + 0.15 k: k = 11: 3.832, 12: 3.8; k = 13 (p = 2): 5.64.  fwd: nkt = 18, 1 x 9 tiles: 11
    # (test_fwd_plan.py: test_dense_inputs_for_the_dense_top)
    "dense_active_nesterov": _case(
        dict(input_size=32, hidden_size=512, output_size=2, S=33, D=12), "dense",
        dict(nstages=4, tm=2, tn=16, blocks=32),
        dict(I=548, H=516, O=4, ho_asked=1, big=1, ks=12, top="plain", ho_gemm="planes", extras="dense", xc_req="dense", own_ws=1),
        dict(ks=11, nkt=18, input="assemble", end="finalize", output="rows"),
        calc_args=dict(flags=0, active=1, dense_inputs=1, fuse_want=0, own_slab_floats=8 * 548 * 516 + 64 * 128 * 516),
        fwd_args=dict(mode=2, advance=0, want=0)),
    # 20 inputs -> a bottom layer of 12 -> 40 hidden units, 6 streams: I = 56, H = 44, O = 4; 16 columns beside the hidden
    # ones, dense: k_extras_dense.  Nothing is deferred on a bottom-layer net.  calc: nkt = 6 -> 6.  fwd: nkt = 2 -> 2
    "bottom_layer": _case(
        dict(input_size=12, hidden_size=40, output_size=3, S=6, D=6, bottom_inputs=20, bottom_rate_scale=0.25), "bottom",
        dict(nstages=1, tm=1, tn=2, blocks=8),
        dict(I=56, H=44, O=4, ho_asked=0, big=0, ks=6, top="plain", ho_gemm="summed", extras="dense", own_ws=0),
        dict(ks=2, nkt=2, input="bottom", advance_first=0, end="finalize", output="rows"),
        calc_args=dict(flags=0, active=1, dense_inputs=1, defer=0),
        fwd_args=dict(mode=2, advance=0, want=0, bottom=20)),
}

TEXT_CASES = [k for k, c in CASES.items() if c["steps"] == "text"]
TWINS = ["resqrt_256_48_5", "north_star_width_1024_64_10"]

# what the twins get in lock step: the one-launch chain (chain_plan.h: chain_segment -- 3 and 4 row tiles of 16 streams,
# 3 x 8 = 24 and 4 x 32 = 128 workgroups at work, the others take a request for the top layer's delta), the fused forward
# launch, and at hidden 1024 k_delta_direct with the update in its epilogue (I / 64 = 16 x 16 tiles, (64 / 4 / 8) x 10 = 20
# iterations: four rings of five)
TWIN_LOCK_STEP = {
    "resqrt_256_48_5": dict(chain=dict(wanted=1, nsegs=1, seg0="0,48,1,0,48,0>232,1", parts_stood=0, uniform=1, ns=2),
                            calc=dict(direct=0, dma=0), fwd=dict(input="inside", hidden="fused", ns=2, left_planes=1)),
    "north_star_width_1024_64_10": dict(chain=dict(wanted=1, nsegs=1, seg0="0,64,1,0,64,0>128,1", parts_stood=0, uniform=1, ns=8),
                                        calc=dict(direct=1, direct_runs=1, direct_fuse=1, dks=1, dn_it=20),
                                        fwd=dict(input="inside", hidden="fused", ns=8, left_planes=1)),
}


def chain_args(c):
    kw = c["kw"]
    return dict(hidden=kw["hidden_size"], nrows=kw["S"], depth=kw["D"])


def calc_args(c):
    kw = c["kw"]
    a = dict(input=kw["input_size"], hidden=kw["hidden_size"], output=kw["output_size"], streams=kw["S"], depth=kw["D"])
    a.update(TEXT_CALC)
    a.update(c["calc_args"])
    return a


def fwd_args(c):
    kw = c["kw"]
    a = dict(input=kw["input_size"], hidden=kw["hidden_size"], output=kw["output_size"], streams=kw["S"])
    a.update(TEXT_FWD)
    a.update(c["fwd_args"])
    return a
