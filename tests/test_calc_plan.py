"""Which kernels a call of ramd_launch_calc_deltas gets, asked of the rule itself (recur_amd/csrc/calc_plan.h) without a
GPU: calc_plan_harness.cpp is compiled with the host compiler alone and prints the plan for a shape, the call's arguments
and the switches in its environment.  The expected values are worked out by hand from the launcher's conditions; I is
1 + input + hidden rounded up to 4, H is hidden + 1 rounded up to 4, O is output rounded up to 4."""
import os
import subprocess

import pytest

import recur_ctypes as rc

ROOT = rc.ROOT
CSRC = os.path.join(ROOT, "recur_amd", "csrc")
HEADS = 0x10000000    # RAMD_RANGES_ARE_HEADS
PENDING = 0x08000000  # RAMD_IMAGES_PENDING
TOP_DONE = 0x40000000  # RAMD_TOP_DONE
BENCH = dict(input=42, hidden=1024, output=42, streams=256, depth=20)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("calc_plan") / "calc_plan_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "calc_plan_harness.cpp"), "-o", exe], check=True)
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


def shape(i, h, o, s, d, **more):
    return dict(input=i, hidden=h, output=o, streams=s, depth=d, **more)


def test_the_header_needs_no_hip():
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-x", "c++",
                    os.path.join(CSRC, "calc_plan.h")], check=True)


def test_the_benchmark_shape(harness):
    p = plan(harness, **BENCH)
    has(p, I=1068, H=1028, O=44, direct=1, dtm=16, dtn=16, drest=44, npw=1, drg=4, dn_it=160, dks=1, direct_fuse=1,
        ho_in_delta=1, fast_its=210, ho_asked=0, xc_req="gather", small=0, ho_gemm="none")
    has(plan(harness, **BENCH, accumulate=1), direct=1, direct_fuse=0, ho_in_delta=0, ho_asked=0)  # it accumulates
    # I = 1068 is 8 whole 128-row tiles plus 44 rows
    has(plan(harness, {"RECUR_AMD_DELTA_DIRECT": "0"}, **BENCH), direct=0, dma=1, has_rest=1, ho_asked=1, dma_rest_in=1)
    has(plan(harness, {"RECUR_AMD_HO_IN_DELTA": "0"}, **BENCH), ho_in_delta=0, ho_asked=1, direct_fuse=1)


def test_smaller_sets_at_hidden_1024(harness):
    # the loop is shorter than 40: no fast share; 32 streams leave half the chain launch idle ((32/32) (1024/32) = 32 <= 128)
    has(plan(harness, **shape(42, 1024, 42, 32, 10)), direct=1, dn_it=10, fast_its=0, ho_in_delta=0, ho_asked=1)


def test_the_k_split_of_the_direct_gemm(harness):
    has(plan(harness, **shape(42, 512, 42, 128, 30)), direct=1, dks=4, dtm=8, dtn=8, npw=2, drg=4, dn_it=120, direct_fuse=0)
    has(plan(harness, **shape(42, 512, 42, 32, 20)), direct=1, dks=4, dn_it=20)  # the smallest set with dks = 4
    has(plan(harness, **shape(42, 704, 42, 32, 10)), direct=1, dks=2, dtm=11, dtn=11, dn_it=10)  # 121 tiles
    has(plan(harness, {"RECUR_AMD_DELTA_DIRECT_SPLIT": "0"}, **shape(42, 512, 42, 128, 30)), direct=0, dma=1)
    # the planes of the split must fit the workspace (here the caller's own): else k_delta_dma
    n = 556 * 516  # I * H
    has(plan(harness, **shape(42, 512, 42, 128, 30), own_slab_floats=4 * n), direct=1, direct_runs=1, own_ws=1)
    has(plan(harness, **shape(42, 512, 42, 128, 30), own_slab_floats=4 * n - 1), direct=1, direct_runs=0, dma=1, own_ws=1)


def test_a_multi_head_text_net(harness):
    # I = 1100: 17 x 16 tiles would be a round of 256 and a round of 16
    has(plan(harness, **shape(75, 1024, 146, 256, 20)), I=1100, direct=1, dtm=16, drest=76, npw=2, drg=8)


def test_below_the_direct_gemm(harness):
    has(plan(harness, **shape(42, 128, 42, 32, 8)), direct=0, dma=1, has_rest=1)


def test_one_stream_of_a_small_net(harness):
    small = shape(42, 99, 42, 1, 30, defer=0)
    has(plan(harness, **small), small=1)
    has(plan(harness, {"RECUR_AMD_BPTT_SMALL": "0"}, **small), small=0)
    has(plan(harness, **small, active=1), small=0)


@pytest.mark.parametrize("s", [BENCH, shape(42, 1024, 42, 32, 10), shape(42, 512, 42, 128, 30), shape(42, 704, 42, 32, 10),
                               shape(75, 1024, 146, 256, 20), shape(42, 128, 42, 32, 8)])
def test_streams_at_different_ring_positions(harness, s):
    has(plan(harness, **s, uniform_idx=-1), direct=0, dma=0)


def test_the_forms_of_the_top_backprop(harness):
    """(Hand-derived like the rows above.  Kernel traces of the launcher before and after the plan was split from it
    showed `plain`, `done` and `sparse` launching what is said here; `ranged` and `heads` were not traced.)"""
    has(plan(harness, **BENCH), top="plain", writeback_first=0)
    has(plan(harness, **BENCH, flags=TOP_DONE), top="done")
    has(plan(harness, **BENCH, ranges=1, flags=PENDING), top="ranged", top_nb=4, writeback_first=1)
    has(plan(harness, **shape(42, 1024, 42, 32, 10), ranges=1), top="ranged", top_nb=8)
    heads = dict(shape(75, 1024, 146, 256, 20), ranges=1, range_stride=132, mheads_alen=73, flags=HEADS | PENDING)
    has(plan(harness, **heads), top="heads", top_nb=66, writeback_first=1, ho_gemm="heads")  # no workspace for the partial products
    # k_top_heads_combine takes the stale entries from the planes: no write-back in front
    has(plan(harness, **heads, mheads_part_floats=256 * 2 * 1028), top="sparse", writeback_first=0)
    has(plan(harness, **heads, mheads_part_floats=256 * 2 * 1028 - 1), top="heads")
    has(plan(harness, {"RECUR_AMD_TOP_SPARSE": "0", "RECUR_AMD_TOP_HEADS": "0"}, **heads, mheads_part_floats=1 << 20), top="ranged")


def test_the_extras_where_the_chain_declines(harness):
    """(Hand-derived.  The same traces showed `control5` and `dense` (with k_bptt_control behind it); `control8`,
    `control9` and `gemm` were not traced.)"""
    has(plan(harness, **BENCH), extras="control5", xc_req="gather")           # (1028 / 4 + 63) / 64 = 5 float4 per thread
    has(plan(harness, **shape(42, 1536, 42, 32, 10)), extras="control8")       # 7
    has(plan(harness, **shape(42, 2048, 42, 32, 10)), extras="control9")       # 9
    has(plan(harness, **shape(40, 1024, 10, 32, 10), dense_inputs=1), extras="dense", xc_req="dense")  # 44 extra columns
    has(plan(harness, **shape(40, 768, 10, 32, 10), dense_inputs=1), extras="dense", xc_req="none")    # (the tail: hidden 512 / 1024)
    has(plan(harness, **shape(100, 1024, 10, 32, 10), dense_inputs=1), extras="gemm", xc_req="none")   # 104 columns > 48
    has(plan(harness, **shape(4, 1024, 10, 32, 10), dense_inputs=1), extras="control5", xc_req="gather")  # a handful: the gather


def test_the_top_layers_delta_where_nobody_takes_it_along(harness):
    off = {"RECUR_AMD_DELTA_DIRECT": "0"}
    has(plan(harness, off, **BENCH), ho_asked=1, ho_gemm="planes_paired")      # if the chain declines: with the rest rows
    has(plan(harness, off, **BENCH, chain_did_ho=1), ho_gemm="none")
    has(plan(harness, off, **BENCH, accumulate=1), ho_asked=0, ho_gemm="paired_summed")
    has(plan(harness, off, **BENCH, active=1), ho_gemm="planes")
    has(plan(harness, off, **BENCH, defer=0, active=1), ho_gemm="summed")
    has(plan(harness, **shape(42, 64, 42, 8, 6)), ho_asked=0, ho_gemm="planes", direct=0, dma=0)  # fewer than 16 streams
