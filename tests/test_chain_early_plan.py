"""Where the one-launch BPTT chain takes its early form (k_chain_persist_early), asked of the rule itself
(recur_amd/csrc/chain_plan.h: chain_early_blocks, and the `early` field chain_segment() gives every launch) without a GPU:
chain_early_harness.cpp is compiled with the host compiler alone.  A segment reads row0,nrows,one,pad>early.

On: hidden 1024 with 32-stream row tiles.  Off: 16-stream tiles (they have no drain beside a burst), padded launches, a
window, hidden 512 and 256 (not measured yet, so left as they were: profiles/NOTES_r20.md, section 4), and everything with RECUR_AMD_CHAIN_EARLY=0."""
import os
import subprocess

import pytest

import recur_ctypes as rc

ROOT = rc.ROOT
CSRC = os.path.join(ROOT, "recur_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "chain_early_harness.cpp")
CXX = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include")]
OFF = {"RECUR_AMD_CHAIN_EARLY": "0"}
WIDE_TILES = {"RECUR_AMD_CHAIN_ONE": "0"}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chain_early") / "chain_early_harness")
    subprocess.run(CXX + [SRC, "-o", exe], check=True)
    return exe


def ask(exe, env=None, **args):
    e = {k: v for k, v in os.environ.items() if not k.startswith("RECUR_AMD_")}
    e.update(env or {})
    out = subprocess.run([exe] + ["%s=%d" % kv for kv in args.items()], env=e, capture_output=True, text=True, check=True).stdout
    d = dict(line.split("=", 1) for line in out.splitlines())
    return {k: int(v) if v.lstrip("-").isdigit() else v for k, v in d.items()}


def segments(p):
    return [p["seg%d" % i] for i in range(p["nsegs"])]


def test_the_rule(harness):
    p = ask(harness, hidden=1024)
    e = p["blocks"]
    assert 1 <= e < 16  # some of the 16 blocks stay behind the flag
    assert (p["rule_full"], p["rule_one"], p["rule_pad"]) == (e, 0, 0)
    for hidden in (512, 256, 2048, 64):
        p = ask(harness, hidden=hidden, nrows=32)
        assert (p["rule_full"], p["rule_one"], p["rule_pad"]) == (0, 0, 0), hidden
    p = ask(harness, OFF, hidden=1024)
    assert (p["rule_full"], p["rule_one"], p["rule_pad"]) == (0, 0, 0)


def test_the_benchmark_shape_and_the_smallest_full_tile(harness):
    e = ask(harness)["blocks"]
    assert segments(ask(harness, hidden=1024, nrows=256)) == ["0,256,0,0>%d" % e]
    assert segments(ask(harness, hidden=1024, nrows=160)) == ["0,160,0,0>%d" % e]  # ten 16-stream tiles > 8 seats
    # up to 128 streams run as 16-stream tiles unless RECUR_AMD_CHAIN_ONE=0: then one 32-stream tile has the early form
    assert segments(ask(harness, hidden=1024, nrows=32)) == ["0,32,1,0>0"]
    assert segments(ask(harness, WIDE_TILES, hidden=1024, nrows=32)) == ["0,32,0,0>%d" % e]
    assert segments(ask(harness, WIDE_TILES, hidden=1024, nrows=32, row0=32, scap=64)) == ["32,32,0,0>%d" % e]
    # more streams than a launch has seats for: every launch of 32-stream tiles has it, the 16 left over do not
    assert segments(ask(harness, hidden=1024, nrows=272)) == ["0,256,0,0>%d" % e, "256,16,1,0>0"]


def test_off_for_small_tiles_pads_windows_and_small_nets(harness):
    assert segments(ask(harness, hidden=1024, nrows=16)) == ["0,16,1,0>0"]      # a 16-stream tile
    assert segments(ask(harness, hidden=1024, nrows=48)) == ["0,48,1,0>0"]      # three of them: still one launch
    assert segments(ask(harness, hidden=1024, nrows=5, scap=16)) == ["0,16,1,1>0"]  # padded to a tile
    assert segments(ask(harness, hidden=1024, nrows=1, row0=3, scap=16)) == ["0,16,1,1>0"]  # a window: stream 3 of a set
    assert segments(ask(harness, hidden=512, nrows=512)) == ["0,512,0,0>0"]
    assert segments(ask(harness, hidden=256, nrows=1024)) == ["0,1024,0,0>0"]


def test_off_with_the_switch(harness):
    assert segments(ask(harness, OFF, hidden=1024, nrows=256)) == ["0,256,0,0>0"]
    assert segments(ask(harness, dict(OFF, **WIDE_TILES), hidden=1024, nrows=32)) == ["0,32,0,0>0"]
    assert segments(ask(harness, {"RECUR_AMD_CHAIN_EARLY": "1"}, hidden=1024, nrows=256)) == ["0,256,0,0>%d" % ask(harness)["blocks"]]


def test_the_switch_is_among_the_fast_paths_to_switch_off():
    lines = open(os.path.join(ROOT, "tools", "all_fast_paths_off.env")).read().split()
    assert "RECUR_AMD_CHAIN_EARLY=0" in lines
