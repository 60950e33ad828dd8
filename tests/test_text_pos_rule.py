"""Where stream j of a training set reads the text at position i of an epoch, asked of the rule itself
(recur_amd/csrc/text_pos_rule.h) without a GPU: text_pos_rule_harness.cpp is compiled with the host compiler alone.

The reference reads text[(i + j * spacing) % (len - 1)] with spacing = (len - 1) / global_count and takes the byte after
it as the target (charmodel-predict.c:273, 295-298).  The rule has the device's form, one conditional subtraction, which
is the same number for 0 <= i <= len - 1 and 0 <= j < global_count; the harness compares the two for every such case and
checks that the target lies inside the text."""
import os
import subprocess

import pytest

import recur_ctypes as rc

ROOT = rc.ROOT
CSRC = os.path.join(ROOT, "recur_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "text_pos_rule_harness.cpp")
CXX = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("text_pos_rule") / "text_pos_rule_harness")
    subprocess.run(CXX + [SRC, "-o", exe], check=True)
    return exe


def ask(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return dict(line.split("=", 1) for line in r.stdout.splitlines())


def test_the_header_needs_no_hip():
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-Wno-unused-function", "-I", CSRC, "-x", "c++",
                    os.path.join(CSRC, "text_pos_rule.h")], check=True)
    subprocess.run(["gcc", "-std=gnu11", "-fsyntax-only", "-Wall", "-Werror", "-Wno-unused-function", "-I", CSRC, "-x", "c",
                    os.path.join(CSRC, "text_pos_rule.h")], check=True)  # char_epoch.c includes it as C


def test_every_small_text_set_stream_and_position(harness):
    """len 2..40, global_count 1..len + 2 (so a spacing of 0 is among them), every stream, every i in 0..len - 1"""
    d = ask(harness, "sweep", 2, 40)
    want = sum((n + 2) * (n + 3) // 2 * n for n in range(2, 41))  # sum over count of count streams, times len positions
    assert (int(d["cases"]), int(d["bad"])) == (want, 0)


def test_a_long_text_at_its_ends(harness):
    n = (1 << 20) + 1
    d = ask(harness, "at", n, 256, 0, n - 2, n - 1)
    assert (int(d["cases"]), int(d["bad"])) == (3 * 256, 0)


def test_a_text_of_one_byte_divides_by_nothing(harness):
    assert ask(harness, "one", 1, 1, 0, 0) == {"offset": "0"}
    assert ask(harness, "one", 1, 3, 2, 0) == {"offset": "0"}
