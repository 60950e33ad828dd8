"""What launch t of rnn_amd_continue_texts does for a row, asked of the rule itself (recur_amd/csrc/continue_rule.h, what
k_texts_continue and the host loop of sample_api.c both ask) without a GPU: continue_rule_harness.cpp is compiled with g++
alone and prints the rule's answer for every launch of a row.  The expected values are a brute-force simulation of the
contract's loop (include/recur_amd.h): feed the prompt symbol by symbol, then draw, feed the pick, draw, ... -- cut into
launches behind every feed, because a forward pass follows a feed.  The row counts of the forward passes are
texts_plan.h's for len = plen + max_len: its harness (tests/texts_plan_harness.c) is asked for the same rows.  And the
refusals and the empty calls of rnn_amd_continue_texts and rnn_amd_char_continue_texts, which come before anything needs a
device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import recur_ctypes as rc
import sample_oracle as so

ROOT = rc.ROOT
CSRC = os.path.join(ROOT, "recur_amd", "csrc")
IDLE, PROMPT, DRAW = 0, 1, 2
CASES = [(plen, max_len) for plen in range(1, 6) for max_len in range(1, 5)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("continue_rule") / "continue_rule_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "continue_rule_harness.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def plan_harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("continue_plan") / "texts_plan_harness")
    subprocess.run(["gcc", "-std=gnu11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "texts_plan_harness.c"), "-o", exe], check=True)
    return exe


def rule(exe, plen, max_len):
    """[(what, index, feeds, on_hid0)] for t = 0 .. plen + max_len"""
    out = subprocess.run([exe, str(plen), str(max_len)], capture_output=True, text=True, check=True).stdout
    return [tuple(int(x) for x in line.split(",")) for line in out.splitlines()]


def simulated(plen, max_len):
    """the contract's loop as a list of operations, cut into launches: a launch ends with the feed the next forward pass
    computes from, or with the last draw"""
    ops = [("feed prompt", i) for i in range(plen - 1)]      # rnn_char_prime's loop
    sym = ("feed prompt", plen - 1)                          # first = prompts[k][plen - 1]
    for i in range(max_len):                                 # rnn_amd_sample_texts's loop
        ops.append(sym)
        ops.append(("draw", i))
        sym = ("feed pick", i)
    launches, now = [], []
    for op in ops:
        now.append(op)
        if op[0].startswith("feed"):
            launches.append(now)
            now = []
    launches.append(now)
    return launches


def test_the_header_is_plain_c_and_cxx_without_hip():
    subprocess.run(["g++", "-fsyntax-only", "-Wall", "-Werror", "-I", CSRC, "-x", "c++",
                    os.path.join(CSRC, "continue_rule.h")], check=True)
    subprocess.run(["gcc", "-std=gnu11", "-fsyntax-only", "-Wall", "-Werror", "-I", CSRC, "-x", "c",
                    os.path.join(CSRC, "continue_rule.h")], check=True)   # (sample_api.c, the host loop, is C)


@pytest.mark.parametrize("plen,max_len", CASES)
def test_the_rule_is_the_contracts_loop(harness, plen, max_len):
    got = rule(harness, plen, max_len)
    want = simulated(plen, max_len)
    assert len(got) == plen + max_len + 1 and len(want) == plen + max_len
    fed, drawn = [], []
    for t, (what, index, feeds, on_hid0) in enumerate(got):
        ops = want[t] if t < len(want) else []
        if what == PROMPT:
            assert ops == [("feed prompt", index)] and feeds == 1
            fed.append(index)
        elif what == DRAW:
            assert ops == ([("draw", index), ("feed pick", index)] if feeds else [("draw", index)])
            drawn.append(index)
        else:
            assert what == IDLE and ops == [] and not feeds
        assert on_hid0 == (1 if t == 0 else 0)                # the first feed is on the net's hidden row, no other
        assert bool(feeds) == (plen + max_len - 1 > t)        # texts_plan_active's condition for len = plen + max_len
    assert fed == list(range(plen))                           # every prompt symbol once, in order
    assert drawn == list(range(max_len))                      # every text index once, in order
    assert got[plen + max_len - 1][:3] == (DRAW, max_len - 1, 0)   # the last draw is not fed
    assert got[plen + max_len] == (IDLE, 0, 0, 0)             # nothing afterwards


def test_rows_fed_after_a_launch_are_the_plans_active_rows(harness, plan_harness):
    lens = [plen + max_len for plen, max_len in CASES]
    out = subprocess.run([plan_harness, "256", ",".join(map(str, lens))], capture_output=True, text=True, check=True).stdout
    d = dict(line.split("=", 1) for line in out.splitlines())
    active = [int(x) for x in d["active0"].split(",")]
    order = [int(x) for x in d["order"].split(",")]
    rules = [rule(harness, plen, max_len) for plen, max_len in CASES]
    assert len(order) == len(CASES) and len(active) == max(lens)      # steps = longest - 1, and one past the end
    for t, a in enumerate(active):
        feeds = [r[t][2] if t < len(r) else 0 for r in rules]
        assert a == sum(feeds)
        assert all(feeds[k] for k in order[:a]) and not any(feeds[k] for k in order[a:])   # ... and they are its prefix
    # one row alone, every case: the wave's steps are the row's forward passes
    for (plen, max_len), r in zip(CASES, rules):
        out = subprocess.run([plan_harness, "256", str(plen + max_len)], capture_output=True, text=True, check=True).stdout
        d = dict(line.split("=", 1) for line in out.splitlines())
        assert [int(x) for x in d["active0"].split(",")] == [x[2] for x in r[:plen + max_len]]
        assert int(d["wave0"].split(",")[2]) == sum(x[2] for x in r)


def test_refusals_and_empty_calls_need_no_device():
    """-1 with nothing written, 0 for nothing to draw, on a machine without a GPU (no compute entry point is reached: with
    a device present the same calls return before they touch it)"""
    lib = rc.bind_char(rc.load_amd())
    orc = rc.load_oracle()
    net = lib.rnn_new(42, 39, 42, rc.FLAG_STANDARD, 1, None, 4, 1e-3, 0.9, 0.0, rc.RELU)
    bottom = lib.rnn_new_with_bottom_layer(42, 16, 39, 42, rc.FLAG_STANDARD, 5, None, 4, 1e-3, 0.9, 0.0, rc.RELU, 0)
    texts = [np.array([3, 4, 5], np.uint8), np.array([6], np.uint8)]
    ptrs = (rc.c_u8_p * 2)(*[rc.u8ptr(t) for t in texts])
    plens = np.array([3, 1], np.int32)
    seeds = np.array([11, 2 ** 40 + 5], np.uint64)
    sp = seeds.ctypes.data_as(C.POINTER(C.c_uint64))
    out = np.full((2, 10), 0xEE, np.uint8)
    lens = np.full(2, -7, np.int32)
    rng = np.full((2, 4), 9, np.uint64)
    rp = rng.ctypes.data_as(C.POINTER(rc.RandCtx))

    def call(net=net, prompts=ptrs, plens=rc.iptr(plens), seeds=sp, n=2, max_len=10, alen=0, head=0, out=rc.u8ptr(out),
             lens=rc.iptr(lens), rng=rp):
        return lib.rnn_amd_continue_texts(net, prompts, plens, seeds, n, max_len, 0.0, -1, alen, head, out, lens, rng)

    def with_prompts(a, b):
        keep = [np.array(a, np.uint8), np.array(b, np.uint8)]
        return keep, (rc.c_u8_p * 2)(*[rc.u8ptr(t) for t in keep])

    # everything rnn_amd_sample_texts refuses
    assert call(net=None) == -1 and call(net=bottom) == -1
    assert call(n=-1) == -1 and call(max_len=-1) == -1
    assert call(seeds=None) == -1 and call(out=None) == -1 and call(lens=None) == -1
    assert call(alen=5) == -1 and call(alen=-14) == -1      # 42 outputs are not heads of 5
    assert call(alen=14, head=3) == -1 and call(alen=14, head=-1) == -1 and call(head=1) == -1
    # ... and what is refused about the prompts
    assert call(prompts=None) == -1 and call(plens=None) == -1
    for bad in (0, -1):
        assert call(plens=rc.iptr(np.array([3, bad], np.int32))) == -1
    assert call(prompts=(rc.c_u8_p * 2)(rc.u8ptr(texts[0]), None)) == -1
    for a, b in (([3, 42, 5], [6]), ([42, 4, 5], [6]), ([3, 4, 5], [255]), ([3, 4, 200], [6])):   # first, middle, last
        keep, bad = with_prompts(a, b)
        assert call(prompts=bad) == -1
    big = np.array([3, 2 ** 31 - 10], np.int32)             # 2^31 - 10 + 10 symbols do not fit an int; the check comes
    assert call(plens=rc.iptr(big)) == -1                   # before the prompt's symbols are read
    assert call(plens=rc.iptr(np.array([2 ** 31 - 1, 1], np.int32)), max_len=1) == -1
    assert np.all(out == 0xEE) and np.all(lens == -7) and np.all(rng == 9)   # nothing written
    # nothing to draw: lengths zeroed, the generators as seeded, no device asked for
    assert call(n=0, prompts=None, plens=None, seeds=None, out=None, lens=None, rng=None) == 0
    assert np.all(lens == -7) and np.all(rng == 9)
    assert call(max_len=0, rng=None) == 0 and list(lens) == [0, 0] and np.all(rng == 9)
    lens[:] = -7
    assert call(max_len=0) == 0 and list(lens) == [0, 0] and np.all(out == 0xEE)
    for k in range(2):
        assert tuple(int(x) for x in rng[k]) == so.words(so.seeded(orc, int(seeds[k])))
    # the refusals come first, also where nothing would be drawn
    assert call(max_len=0, plens=rc.iptr(np.array([3, 0], np.int32))) == -1
    # the character layer: a prompt that encodes to nothing is refused, refusals pass through, too little room writes nothing
    alphabet = rc.default_text_alphabet(lib)
    bufs = [C.create_string_buffer(b"\x55" * 8, 8) for _ in range(2)]
    dest = (C.c_char_p * 2)(*[C.cast(b, C.c_char_p) for b in bufs])
    nbytes = np.full(2, -7, np.int32)

    def char_call(net=net, prompts=(b"the ", b"a"), n=2, byte_len=8):
        ps = (C.c_char_p * 2)(*prompts)
        pb = np.array([len(p) if p is not None else 0 for p in prompts], np.int32)
        for b in bufs:
            b.raw = b"\x55" * 8
        nbytes[:] = -7
        return lib.rnn_amd_char_continue_texts(net, alphabet, ps, rc.iptr(pb), sp, n, 5, 0.0, -1, dest, byte_len, rc.iptr(nbytes))

    assert char_call(prompts=(b"the ", b"")) == -1
    assert list(nbytes) == [0, 0] and all(b.raw[0] == 0 and b.raw[1:] == b"\x55" * 7 for b in bufs)
    assert char_call(prompts=(None, b"a")) == -1 and list(nbytes) == [0, 0]
    assert char_call(net=bottom) == -1 and list(nbytes) == [0, 0]
    assert char_call(n=-1) == -1
    assert char_call(n=0) == 0 and list(nbytes) == [-7, -7]
    assert char_call(byte_len=1) == 0
    assert list(nbytes) == [0, 0] and all(b.raw[0] == 0 and b.raw[1:] == b"\x55" * 7 for b in bufs)
    lib.rnn_char_free_alphabet(alphabet)
    lib.rnn_delete_net(bottom)
    lib.rnn_delete_net(net)
