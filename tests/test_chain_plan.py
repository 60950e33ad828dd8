"""Which launches the BPTT chain (ramd_chain_steps) gets, asked of the rule itself (recur_amd/csrc/chain_plan.h) without a
GPU: chain_plan_harness.cpp is compiled with the host compiler alone and prints the plan for a shape, the call's rows and
the switches in its environment.  The expected values are worked out by hand from the conditions the launcher had before
the plan was split from it.

The one-launch chain (k_chain_persist): hidden 1024 / 512 / 256 has nt = 32 / 16 / 8 column tiles and so 8 / 16 / 32 row
tiles ("seats") per launch, of 16 streams where all that is left fits one launch (and is no multiple of 32, or
RECUR_AMD_CHAIN_ONE), else of 32.  A segment reads row0,nrows,one,pad,nvalid,vlo>workers,idle_only: with busy = row tiles x
nt workgroups at work, a request for the top layer's delta goes to the 256 - busy others where they are at least 128,
else to all 256.  The per-step form's workgroups: blocks = ceil(tn / 8) * 8 * tm."""
import os
import subprocess

import pytest

import recur_ctypes as rc

ROOT = rc.ROOT
CSRC = os.path.join(ROOT, "recur_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "chain_plan_harness.cpp")
CXX = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include")]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chain_plan") / "chain_plan_harness")
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


def call(hidden, nrows, depth, **more):
    return dict(hidden=hidden, nrows=nrows, depth=depth, **more)


def segments(p, *segs):
    """all of the plan's one-launch segments, and that ramd_chain_steps returns 0 where they stand"""
    assert [p.get("seg%d" % i) for i in range(p["nsegs"])] == list(segs)
    assert p["parts_stood"] == (0 if segs else p["parts"])


# 256 streams at hidden 1024 a launch per step: 1024 / 64 = 16 stages and 16 column tiles of 64; 4 x 16 = 64 tiles of 64
# streams (< 192) but 8 x 16 = 128 of 32 streams: 32 x 64 tiles; blocks = 2 * 8 * 8
BENCH_STEPS = dict(form="wide", ns=16, mt=32, tm=8, tn=16, blocks=128, parts=16)


def test_the_header_needs_no_hip():
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-x", "c++",
                    os.path.join(CSRC, "chain_plan.h")], check=True)


def test_the_benchmark_shape(harness):
    # 16 tiles of 16 streams > 8 seats: 32-stream tiles, 8 x 32 = 256 workgroups at work
    p = plan(harness, **call(1024, 256, 20))
    has(p, wanted=1, chain_rows=256, windowed=0, **BENCH_STEPS)
    segments(p, "0,256,0,0,256,0>256,0")


def test_sets_of_whole_tiles_in_one_launch(harness):
    # 2 tiles of 16 <= 8 seats: 16-stream tiles, busy 2 x 32 = 64.  Per step: 32 % 64 != 0 and 1 x 16 tiles of 32 streams
    # < 128: k_chain_main, 1024 / 128 = 8 whole stages, tm = 1, tn = 32, blocks = 4 * 8 * 1
    p = plan(harness, **call(1024, 32, 20))
    has(p, form="main", uniform=1, ns=8, nstages=8, mt=32, tm=1, tn=32, blocks=32, parts=32)
    segments(p, "0,32,1,0,32,0>192,1")
    # 8 tiles of 16 = 8 seats: busy 8 x 32 = 256, nobody idle.  Per step: 2 x 16 = 32 tiles of 64 streams, 4 x 16 = 64 of 32
    p = plan(harness, **call(1024, 128, 20))
    has(p, form="main", ns=8, tm=4, tn=32, blocks=128)
    segments(p, "0,128,1,0,128,0>256,0")
    # hidden 256: 32 seats, nt = 8.  80 streams: 5 tiles of 16, busy 40; 256 / 128 = 2 stages, tm = 3, tn = 8
    p = plan(harness, **call(256, 80, 7))
    has(p, form="main", ns=2, nstages=2, tm=3, tn=8, blocks=24, parts=8)
    segments(p, "0,80,1,0,80,0>216,1")
    # 640 streams: 40 tiles of 16 > 32 seats: 20 tiles of 32 (<= 32 seats) in one launch, busy 160: 96 idle < 128
    p = plan(harness, **call(256, 640, 6))
    has(p, form="main", ns=2, tm=20, tn=8, blocks=160)
    segments(p, "0,640,0,0,640,0>256,0")


def test_more_rows_than_one_launch_seats(harness):
    # 512 streams: two launches of 8 x 32.  Per step: 8 x 16 = 128 tiles of 64 streams (< 192), 16 x 16 = 256 of 32
    p = plan(harness, **call(1024, 512, 20))
    has(p, form="wide", ns=16, mt=32, tm=16, tn=16, blocks=256, parts=16)
    segments(p, "0,256,0,0,256,0>256,0", "256,256,0,0,256,0>256,0")
    # 272 = 17 tiles of 16: 272 & ~31 = 256 in 32-stream tiles, then the last 16 alone (busy 32).  Per step: tm = 9
    p = plan(harness, **call(1024, 272, 3))
    has(p, form="main", ns=8, tm=9, tn=32, blocks=288)
    segments(p, "0,256,0,0,256,0>256,0", "256,16,1,0,16,0>224,1")
    # 144 = 9 tiles of 16 > 8 seats: 128 in 32-stream tiles (busy 4 x 32 = 128: 128 idle), then 16
    p = plan(harness, **call(1024, 144, 4))
    has(p, form="main", ns=8, tm=5, tn=32, blocks=160)
    segments(p, "0,128,0,0,128,0>128,1", "128,16,1,0,16,0>224,1")
    # the largest set the callers make: 13,824 = 54 x 256
    p = plan(harness, **call(1024, 13824, 20))
    has(p, nsegs=54, seg0="0,256,0,0,256,0>256,0", seg53="13568,256,0,0,256,0>256,0", parts_stood=0)


def test_sets_that_are_not_whole_tiles_run_padded(harness):
    # 250 -> 256 rows: 16 tiles > 8 seats; 250 & ~31 = 224 real rows in 32-stream tiles (busy 7 x 32 = 224), then 32 rows
    # in 16-stream tiles of which 26 are real (busy 2 x 32).  Per step: 250 is no multiple of 32: k_chain_main, tm = 8
    p = plan(harness, **call(1024, 250, 3, scap=256))
    has(p, chain_rows=256, form="main", ns=8, tm=8, tn=32, blocks=256)
    segments(p, "0,224,0,0,224,0>256,0", "224,32,1,1,26,0>192,1")
    # one stream: one 16-row tile
    p = plan(harness, **call(1024, 1, 5, scap=16))
    has(p, chain_rows=16, form="main", ns=8, tm=1, tn=32, blocks=32)
    segments(p, "0,16,1,1,1,0>224,1")
    # hidden 512: 16 seats, nt = 16; 21 -> 32 rows, busy 2 x 16.  Per step: 4 stages, tn = 16, blocks = 2 * 8 * 1
    p = plan(harness, **call(512, 21, 4, scap=32))
    has(p, chain_rows=32, form="main", ns=4, nstages=4, tm=1, tn=16, blocks=16, parts=16)
    segments(p, "0,32,1,1,21,0>224,1")
    # no rows above the set to run over: a launch per step
    p = plan(harness, **call(1024, 250, 3, scap=250))
    has(p, wanted=0, chain_rows=250)
    segments(p)


def test_sets_that_start_inside_a_tile_run_windowed(harness):
    # rows 4..23 of 48: the tiles from row 0, 32 rows of which [4, 24) are the call's; busy 2 x 8
    p = plan(harness, **call(256, 20, 6, row0=4, scap=48))
    has(p, windowed=1, form="main", ns=2, tm=1, tn=8, blocks=8)
    segments(p, "0,32,1,1,24,4>240,1")
    # row 5 of 16 (its own rows cannot be padded: 5 + 16 > 16; the window asks)
    p = plan(harness, **call(256, 1, 6, row0=5, scap=16))
    has(p, windowed=1, chain_rows=1, form="main", ns=2, blocks=8)
    segments(p, "0,16,1,1,6,5>248,1")
    # rows 14..16 straddle two tiles
    p = plan(harness, **call(256, 3, 6, row0=14, scap=32))
    has(p, windowed=1, form="main", ns=2)
    segments(p, "0,32,1,1,17,14>240,1")
    # rows 250..269 of 272 at hidden 1024: from row 240, two tiles, busy 2 x 32
    p = plan(harness, **call(1024, 20, 3, row0=250, scap=272))
    has(p, windowed=1, form="main", ns=8, tm=1, blocks=32)
    segments(p, "240,32,1,1,30,10>192,1")
    # a window of more tiles than a launch has seats (rows 4..259: 17 tiles > 8) is none: the call's own 256 rows, from row 4
    p = plan(harness, **call(1024, 256, 3, row0=4, scap=272))
    has(p, wanted=1, windowed=0)
    segments(p, "4,256,0,0,256,0>256,0")
    # ... and where its own rows do not qualify either (200 -> 208 rows would end at 212 > 208) the launcher has still asked
    # whether the chain is available -- the probe runs for this call, as it always did -- and runs a launch per step
    p = plan(harness, **call(1024, 200, 3, row0=4, scap=208))
    has(p, wanted=1, windowed=0, chain_rows=200)
    segments(p)
    # a window that would end above Scap (rows 20..29 of 30 -> 16..31)
    p = plan(harness, **call(256, 10, 6, row0=20, scap=30))
    has(p, wanted=0, windowed=0)
    segments(p)


def test_without_sixteen_stream_tiles_for_multiples_of_32(harness):
    off = {"RECUR_AMD_CHAIN_ONE": "0"}
    # 64 streams: 2 tiles of 32, busy 64.  Per step: 1 x 16 tiles of 64 streams, 2 x 16 of 32: k_chain_main, tm = 2
    p = plan(harness, off, **call(1024, 64, 20))
    has(p, form="main", ns=8, tm=2, tn=32, blocks=64)
    segments(p, "0,64,0,0,64,0>192,1")
    # 150 -> 160 rows: 128 real rows in 32-stream tiles; of the last 32 rows 22 are real: no whole real 32-stream tile
    # (22 & ~31 = 0), so 16-stream tiles after all
    p = plan(harness, off, **call(1024, 150, 4, scap=160))
    has(p, form="main", ns=8)
    segments(p, "0,128,0,0,128,0>128,1", "128,32,1,1,22,0>192,1")


def test_where_the_one_launch_chain_does_not_take_the_call(harness):
    # deeper than 60 steps; not available (the probe failed or a launch gave up); switched off: the same per-step form
    p = plan(harness, **call(1024, 256, 61))
    has(p, wanted=0, **BENCH_STEPS)
    segments(p)
    p = plan(harness, **call(1024, 256, 20, available=0))
    has(p, wanted=1, **BENCH_STEPS)
    segments(p)
    p = plan(harness, {"RECUR_AMD_CHAIN_PERSIST": "0"}, **call(1024, 256, 20))
    has(p, wanted=0, **BENCH_STEPS)
    segments(p)
    # ... and with 512 streams: 8 x 16 = 128 tiles of 64 streams (< 192) ... with 768: 12 x 16 = 192: 64 x 64 tiles
    has(plan(harness, {"RECUR_AMD_CHAIN_PERSIST": "0"}, **call(1024, 512, 3)), form="wide", ns=16, mt=32, tm=16, tn=16, blocks=256)
    has(plan(harness, {"RECUR_AMD_CHAIN_PERSIST": "0"}, **call(1024, 768, 3)), form="wide", ns=16, mt=64, tm=12, tn=16, blocks=192)
    # streams at different ring positions: k_chain_main<false>, stages counted at run time
    # (run on the GPU by test_gpu_staggered_rings.py: test_a_staggered_text_step_matches_the_oracle, whose shapes
    # test_staggered_rings_cpu.py pins in the same way)
    p = plan(harness, **call(1024, 256, 20, uniform_idx=-1))
    has(p, wanted=0, form="main", uniform=0, ns=0, nstages=8, tm=8, tn=32, blocks=256, parts=32)
    segments(p)


def test_wide_nets_a_launch_per_step(harness):
    # hidden 2048: 32 stages and 32 column tiles of 64.  256 streams: 4 x 32 = 128 tiles of 64 streams (< 192), 8 x 32 = 256 of 32
    p = plan(harness, **call(2048, 256, 7))
    has(p, wanted=0, form="wide", ns=32, mt=32, tm=8, tn=32, blocks=256, parts=32)
    segments(p)
    # 160 streams: 2 x 32 = 64 tiles of 64 streams, 5 x 32 = 160 of 32
    has(plan(harness, **call(2048, 160, 4)), form="wide", ns=32, mt=32, tm=5, tn=32, blocks=160)
    # 512 streams: 8 x 32 = 256 tiles of 64 streams (>= 192): 64 x 64 tiles
    has(plan(harness, **call(2048, 512, 10)), form="wide", ns=32, mt=64, tm=8, tn=32, blocks=256)
    # hidden 1536: 24 stages; 8 x 24 = 192 tiles of 64 streams; blocks = 3 * 8 * 8
    has(plan(harness, **call(1536, 512, 4)), form="wide", ns=24, mt=64, tm=8, tn=24, blocks=192, parts=24)
    # ... and 192 streams: 3 x 24 = 72 tiles of 64 streams, 6 x 24 = 144 of 32; blocks = 3 * 8 * 6
    has(plan(harness, **call(1536, 192, 3)), form="wide", ns=24, mt=32, tm=6, tn=24, blocks=144, parts=24)
    has(plan(harness, **call(1536, 160, 3)), form="main", ns=0, nstages=12, tm=5, tn=48, blocks=240)  # 5 x 24 = 120 < 128
    # 32 streams: 1 x 32 tiles of 32 streams < 128: k_chain_main, 2048 / 128 = 16 stages, tn = 64
    has(plan(harness, **call(2048, 32, 5)), form="main", uniform=1, ns=16, nstages=16, tm=1, tn=64, blocks=64, parts=64)
    # 2112 = 16.5 x 128: 17 stages, the last partial: the form for any number; tn = 66, blocks = 9 * 8 * 1
    has(plan(harness, **call(2112, 2, 3, scap=16)), wanted=0, form="main", uniform=1, ns=0, nstages=17, tn=66, blocks=72, parts=66)
    has(plan(harness, **call(39, 3, 70, scap=16)), wanted=0, form="main", uniform=1, ns=0, nstages=1, tn=2, blocks=8, parts=2)


def test_wide_nets_with_the_wide_forms_switched_off(harness):
    half_off, wide_off = {"RECUR_AMD_CHAIN_WIDE_HALF": "0"}, {"RECUR_AMD_CHAIN_WIDE": "0"}
    # 256 streams: 4 x 32 = 128 tiles of 64 streams are enough for the 64 x 64 form; blocks = 4 * 8 * 4
    has(plan(harness, half_off, **call(2048, 256, 7)), form="wide", ns=32, mt=64, tm=4, tn=32, blocks=128, parts=32)
    # 160 is no multiple of 64: k_chain_main, tm = 5, tn = 64, blocks = 8 * 8 * 5
    has(plan(harness, half_off, **call(2048, 160, 4)), form="main", ns=16, tm=5, tn=64, blocks=320, parts=64)
    has(plan(harness, half_off, **call(2048, 512, 10)), form="wide", ns=32, mt=64, tm=8, tn=32, blocks=256)  # as it was
    has(plan(harness, wide_off, **call(2048, 256, 7)), form="main", uniform=1, ns=16, nstages=16, tm=8, tn=64, blocks=512, parts=64)
    has(plan(harness, wide_off, **call(2048, 160, 4)), form="main", ns=16, tm=5, tn=64, blocks=320)
    has(plan(harness, wide_off, **call(2048, 512, 10)), form="main", ns=16, tm=16, tn=64, blocks=1024, parts=64)
    # the benchmark shape's fall-back: 8 stages, tm = 8, tn = 32
    has(plan(harness, wide_off, **call(1024, 256, 20, available=0)), form="main", ns=8, tm=8, tn=32, blocks=256, parts=32)
    # 64 tiles of 64 streams < 128 without the half form
    has(plan(harness, half_off, **call(1024, 256, 20, available=0)), form="main", ns=8, blocks=256)
