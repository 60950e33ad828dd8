"""What the residency probe's answer means for the launches whose 256 workgroups wait for one another (k_chain_persist,
k_fwd_top), asked of the rule itself (recur_amd/csrc/coop_rule.h) without a GPU: coop_rule_harness.cpp is compiled with
the host compiler alone.

The cases are derived by hand from what the seat table is: the probe's 256 workgroups, one per CU, each name their XCD
and their CU's hardware number; per XCD the 32 numbers (low 8 bits) in ascending order are seats 0 .. 31, every other
entry says "no such CU" (every byte 0xff); an XCD with other than 32 workgroups, or one number twice, gives no table.
"In turn": workgroup i on XCD i % 8.  "Resident": nobody timed out and all 256 arrived.  The seat mode of a chain launch
is 2 with the table, 1 only on request with the workgroups in turn and no side stream, otherwise 0 (tickets).  A flag
sequence starts over at 2^25 (the chain: flags are seq * 64 + step) and 2^30 (the forward + top launch)."""
import itertools
import os
import random
import subprocess

import pytest

import recur_ctypes as rc

ROOT = rc.ROOT
CSRC = os.path.join(ROOT, "recur_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "coop_rule_harness.cpp")
CXX = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include")]
NO_SEAT_OK = {"unnamed_ok%d" % x: "1" for x in range(8)}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("coop_rule") / "coop_rule_harness")
    subprocess.run(CXX + [SRC, "-o", exe], check=True)
    return exe


def ask(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, check=True).stdout
    return dict(line.split("=", 1) for line in out.splitlines())


def table(exe, pairs, arrived=256, fail=0):
    d = ask(exe, "table", arrived, fail, *["%d,%d" % p for p in pairs])
    seats = None
    if d["table"] == "1":
        assert {k: d[k] for k in NO_SEAT_OK} == NO_SEAT_OK  # every entry is a seat below 32 or "no such CU"
        seats = [dict((int(k), int(v)) for k, v in (e.split(":") for e in d["seats%d" % x].split())) for x in range(8)]
    return int(d["resident"]), int(d["in_turn"]), seats


def healthy(keys=range(32)):
    """workgroup i on XCD i % 8; the four workgroups i = 8 q + x of XCD x take its CU numbers in order"""
    keys = list(keys)
    return [(i % 8, keys[i // 8]) for i in range(256)]


def test_the_header_needs_no_hip():
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", CSRC, "-x", "c++", os.path.join(CSRC, "coop_rule.h")], check=True)
    subprocess.run(["gcc", "-std=gnu11", "-fsyntax-only", "-I", CSRC, "-x", "c", os.path.join(CSRC, "coop_rule.h")],
                   check=True)  # engine.c includes it as C


def test_a_healthy_probe(harness):
    resident, in_turn, seats = table(harness, healthy())
    assert (resident, in_turn) == (1, 1)
    assert seats == [{k: k for k in range(32)}] * 8  # seat = key


def test_the_dispatch_order_does_not_matter(harness):
    pairs = healthy()
    random.Random(18).shuffle(pairs)
    assert [x for x, _ in pairs] != [i % 8 for i in range(256)]
    resident, in_turn, seats = table(harness, pairs)
    assert (resident, in_turn) == (1, 0)
    assert seats == table(harness, healthy())[2]  # the identical table


def test_keys_with_gaps_take_seats_in_ascending_order(harness):
    keys = list(range(16)) + list(range(32, 48))  # a shader-array bit between the two halves
    _, in_turn, seats = table(harness, healthy(reversed(keys)))  # (dealt in descending order: the sort is the rule's)
    assert in_turn == 1
    assert seats == [{k: n for n, k in enumerate(keys)}] * 8
    # bits above the low 8 of a key are not part of the CU's number
    assert table(harness, [(x, k | 0x300) for x, k in healthy(keys)])[2] == seats


def test_an_xcd_short_of_workgroups_gives_no_table(harness):
    pairs = healthy()
    i = pairs.index((3, 31))
    pairs[i] = (5, 200)  # XCD 3 has 31 workgroups, XCD 5 has 33, all keys distinct
    resident, in_turn, seats = table(harness, pairs)
    assert (resident, in_turn, seats) == (1, 0, None)


def test_a_repeated_key_gives_no_table(harness):
    pairs = healthy()
    pairs[pairs.index((6, 7))] = (6, 8)  # two workgroups of XCD 6 on CU number 8, still 32 of them
    resident, in_turn, seats = table(harness, pairs)
    assert (resident, in_turn, seats) == (1, 1, None)


def test_resident_means_everybody_arrived_and_nobody_timed_out(harness):
    assert table(harness, healthy(), arrived=255)[0] == 0
    assert table(harness, healthy(), fail=1)[0] == 0
    assert table(harness, healthy(), arrived=255, fail=1)[0] == 0
    assert table(harness, healthy(), arrived=256, fail=0)[0] == 1


def test_the_seat_mode_of_a_chain_launch(harness):
    for tbl, static, in_turn, side in itertools.product((0, 1), repeat=4):
        want = 2 if tbl else 1 if (static and in_turn and not side) else 0
        assert int(ask(harness, "mode", tbl, static, in_turn, side)["mode"]) == want, (tbl, static, in_turn, side)


def test_a_flag_sequence_starts_over_exactly_at_its_limit(harness):
    for name, limit in (("chain", 1 << 25), ("fwd_top", 1 << 30)):
        below, at = ask(harness, "seq", limit - 1), ask(harness, "seq", limit)
        assert int(below[name + "_limit"]) == limit
        assert (int(below[name + "_starts_over"]), int(at[name + "_starts_over"])) == (0, 1)
        assert int(ask(harness, "seq", 0)[name + "_starts_over"]) == 0
        # the launcher asks, then counts up: the largest flag in use belongs to the limit itself
        assert int(below[name + "_largest_flag"]) < 1 << 32
    assert int(below["chain_epoch"]) == 64
    assert int(ask(harness, "seq", (1 << 25) - 1)["chain_largest_flag"]) == (1 << 25) * 64 + 63
    assert int(ask(harness, "seq", (1 << 30) - 1)["fwd_top_largest_flag"]) == 1 << 30


def test_the_abort_codes_keep_their_numbers(harness):
    assert ask(harness, "seq", 0)["abort_codes"] == "1,2,6,7"  # chain, chain off its XCD, exchange barrier, forward + top
