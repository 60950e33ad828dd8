"""Which text steps take their forward pass and top layer as ONE launch (k_fwd_top), asked of the rule itself
(recur_amd/csrc/fwd_top_plan.h) without a GPU: fwd_top_plan_harness.cpp is compiled with the host compiler alone.

The table is derived by hand from what the launch is: 256 workgroups, one per CU; the 32 column-tile workgroups of a
32-stream row tile on one XCD, workgroup j of them also stream j's top layer.  So hidden 1024 (32 column tiles = 32
streams), whole row tiles at one ring position, at most eight (one per XCD), text input, no noise, no bottom layer, the
shape k_text_top2 takes (o_size a multiple of 4 up to 64), the residency probe passed with its seat table, and the
process not on tickets (recur_amd/csrc/coop_rule.h: SeatRule; tests/test_coop_rule.py asks that rule itself).

And the build-time promise of the kernel: its hidden-1024 instantiation needs no scratch memory and no accumulation
registers as spill space (sixteen waves a workgroup leave each wave 128 registers)."""
import os
import re
import subprocess

import pytest

import recur_ctypes as rc

ROOT = rc.ROOT
CSRC = os.path.join(ROOT, "recur_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "fwd_top_plan_harness.cpp")
CXX = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include")]
HIPCC = "/opt/rocm/bin/hipcc"
ONE_HOT, DENSE, TEXT = 1, 2, 3  # RAMD_IN_*
WHOLE, TEXT_TOP = 0, 1          # RAMD_FWD_*


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fwd_top_plan") / "fwd_top_plan_harness")
    subprocess.run(CXX + [SRC, "-o", exe], check=True)
    return exe


def takes(exe, env=None, **args):
    e = {k: v for k, v in os.environ.items() if not k.startswith("RECUR_AMD_")}
    e.update(env or {})
    out = subprocess.run([exe] + ["%s=%d" % kv for kv in args.items()], env=e, capture_output=True, text=True, check=True).stdout
    d = dict(line.split("=", 1) for line in out.splitlines())
    return int(d["takes"])


def test_the_header_needs_no_hip():
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-x", "c++",
                    os.path.join(CSRC, "fwd_top_plan.h")], check=True)


def test_the_calls_that_take_the_one_launch(harness):
    assert takes(harness) == 1                                   # the north star: 1024 hidden, 256 streams, 42 symbols
    assert takes(harness, streams=32) == 1                       # one row tile
    assert takes(harness, streams=64) == 1                       # two XCDs
    assert takes(harness, streams=32, input=64, output=64) == 1  # o_size 64: the softmax wave's edge
    assert takes(harness, streams=64, row0=32) == 1              # the second row tile of a 64-stream training set
    assert takes(harness, streams=224) == 1                      # seven row tiles, one XCD idle


def test_the_calls_that_keep_the_two_launches(harness):
    assert takes(harness, streams=16) == 0                        # half a row tile
    assert takes(harness, streams=48) == 0                        # one and a half
    assert takes(harness, streams=64, row0=16, nrows=32) == 0     # a row tile that starts inside another
    assert takes(harness, streams=288) == 0                       # nine row tiles: eight XCDs
    assert takes(harness, hidden=512) == 0                        # 16 column tiles
    assert takes(harness, hidden=2048) == 0
    assert takes(harness, noise=1) == 0                           # presynaptic noise
    assert takes(harness, uniform_idx=-1) == 0                    # staggered rings
    assert takes(harness, tickets=1) == 0                         # side stream, RCCL group
    assert takes(harness, resident=0) == 0                        # the probe failed, or a launch has given up
    assert takes(harness, table=0) == 0                           # no seat table
    assert takes(harness, bottom=20) == 0                         # a bottom layer
    assert takes(harness, input=68, output=68) == 0               # o_size 68 > 64: k_text_top, not k_text_top2
    assert takes(harness, mode=ONE_HOT) == 0
    assert takes(harness, want=WHOLE) == 0                        # a pass that goes on to a generic output layer
    assert takes(harness, advance=0) == 0
    assert takes(harness, rows_built=1) == 0


def test_the_switches(harness):
    assert takes(harness, {"RECUR_AMD_FWD_TOP": "0"}) == 0
    assert takes(harness, {"RECUR_AMD_FWD_TOP": "1"}) == 1
    assert takes(harness, {"RECUR_AMD_TEXT_TOP2": "0"}) == 0      # the top's body is k_text_top2's
    assert takes(harness, {"RECUR_AMD_NO_TEXT_TOP": "1"}) == 0
    assert takes(harness, {"RECUR_AMD_NO_FWD_FUSED": "1"}) == 0   # the forward half is k_fwd_fused's
    # the chain's checked mode reads, clears and survives the shared abort word behind every chain launch: a give-up of
    # this launch would be taken for the chain's, so the mode keeps the two launches
    assert takes(harness, {"RECUR_AMD_CHAIN_CHECK": "1"}) == 0
    assert takes(harness, {"RECUR_AMD_CHAIN_TEST_GIVEUP": "2"}) == 0
    assert takes(harness, {"RECUR_AMD_CHAIN_TEST_GIVEUP": "1"}) == 1  # (the probe's failure branch: `resident` says it)
    env = dict(line.strip().split("=", 1) for line in open(os.path.join(ROOT, "tools", "all_fast_paths_off.env"))
               if line.strip() and not line.startswith("#"))
    assert env.get("RECUR_AMD_FWD_TOP") == "0"


def test_the_kernel_needs_no_scratch_and_no_accumulation_registers(tmp_path):
    # (no skip where hipcc is missing: the library is built with it, and PARK's register economy in fwd_fused_tile hangs on
    # the compiler -- this test is its only guard)
    asm = str(tmp_path / "kernels_forward.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(CSRC, "kernels_forward.hip"), "-S", "--cuda-device-only", "-o", asm],
                   check=True, capture_output=True)
    text = open(asm).read()
    syms = re.findall(r"^(_Z\d+k_fwd_topILi8E\w*):", text, re.M)
    assert len(syms) == 1, syms
    body = text.split("\n" + syms[0] + ":", 1)[1].split(".Lfunc_end", 1)[0]
    code = [line.split(";")[0] for line in body.splitlines()]
    assert sum("v_mfma_f32_32x32x2" in line for line in code) == 128  # (this IS the kernel: 8 stages x 16)
    assert not [line for line in code if "scratch_" in line]
    assert not [line for line in code if "v_accvgpr" in line]
    meta = text.split(".amdhsa_kernel " + syms[0], 1)[1].split(".end_amdhsa_kernel", 1)[0]
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1)) == 0
    assert int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", meta).group(1)) <= 128
