"""How the per-text hidden states of rnn_amd_run_texts_from, rnn_amd_trace_texts_from and rnn_amd_continue_texts_from
travel between the caller's arrays (the caller's order) and a wave's state rows (texts_plan.h's order), asked of the rule
itself (recur_amd/csrc/texts_states.h) without a GPU: texts_states_harness.cpp is compiled with g++ alone, packs, "runs"
(0.5 added to the elements that carry a state) and unpacks every wave, fills the texts without a row, and writes what
the staging buffer and the caller's arrays held.  The expected values are a numpy restatement of the contract
(include/recur_amd.h) below; the same restatement with one rule broken at a time shows that the cases would notice.  The
same program runs under the address and undefined-behaviour sanitizers (it has its own main; nothing is preloaded).
And, through the library, the refusals of the three calls and their early returns, which come before anything needs a
device.  What the calls compute is tests/test_gpu_texts_states.py's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import recur_ctypes as rc
from recur_amd.drivers import continue_texts_from, run_texts_from, trace_texts_from

ROOT = rc.ROOT
CSRC = os.path.join(ROOT, "recur_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "texts_states_harness.cpp")
CXX = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
SENTINEL = np.float32(-7777.0)
LENS300 = [k % 41 for k in range(300)]          # two waves of 256, ties, 16 texts that take no row
CASES = [(256, 132, 130, LENS300), (256, 104, 99, LENS300), (7, 44, 39, LENS300), (7, 8, 5, [5, 0, 2, 600, 1, 2, 64, 600]),
         (256, 44, 39, [1, 0, 1]), (3, 8, 7, [9, 9, 9, 9, 9, 9, 9])]   # (wave width, h_size, hidden_size, lens)


def build(tmp_path_factory, name, extra=()):
    exe = str(tmp_path_factory.mktemp(name) / "texts_states_harness")
    subprocess.run(CXX + list(extra) + [SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build(tmp_path_factory, "texts_states")


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return build(tmp_path_factory, "texts_states_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def ask(exe, wave_width, width, hidden, mode, lens):
    r = subprocess.run([exe, str(wave_width), str(width), str(hidden), mode, ",".join(map(str, lens))], capture_output=True)
    assert r.returncode == 0, r.stderr[-3000:]
    flat = np.frombuffer(r.stdout, np.float32)
    n, rows = len(lens), sum(1 for x in lens if x >= 2)
    assert flat.size == (rows + n + (0 if mode == "null" else n)) * width
    staged = flat[:rows * width].reshape(rows, width)
    h_out = flat[rows * width:(rows + n) * width].reshape(n, width)
    h_in = None if mode == "null" else flat[(rows + n) * width:].reshape(n, width)
    return staged, h_out, h_in


def start_arrays(n, width):
    h_in = (1000.0 * np.arange(n)[:, None] + np.arange(width)[None, :]).astype(np.float32)
    return h_in, (-1.0 - np.arange(width)).astype(np.float32)


def restated(wave_width, width, hidden, mode, lens, broken=None):
    """the contract in numpy: (what every wave's pack stages, h_out).  broken: one rule left out"""
    n = len(lens)
    h_in, fallback = start_arrays(n, width)
    carries = slice(1, hidden + 1)

    def start_state(k):
        row = np.zeros(width, np.float32)           # element 0 and the padding are never read from h_in
        row[carries] = (fallback if mode == "null" else h_in[k])[carries]
        return row

    rows = [k for k in range(n) if lens[k] >= 2]
    if broken != "caller order as plan order":
        rows.sort(key=lambda k: (-lens[k], k))      # longest first, the caller's order among equals
    h_out = np.full((n, width), SENTINEL) if mode != "inplace" else h_in.copy()
    starts = [start_state(k) for k in range(n)]     # (taken before an update in place overwrites anything)
    staged = []
    for w0 in range(0, len(rows), wave_width):
        wave = rows[w0:w0 + wave_width]
        if broken == "wave offset dropped":
            wave = rows[:len(wave)]
        st = np.stack([starts[k] for k in wave])
        staged.append(st.copy())
        st[:, carries] += np.float32(0.5)           # the device's part
        for j, k in enumerate(wave):
            h_out[k] = st[j]
    if broken != "no-row fill skipped":
        for k in range(n):
            if lens[k] < 2:
                h_out[k] = starts[k]
    return (np.concatenate(staged) if staged else np.zeros((0, width), np.float32)), h_out


def check(exe):
    for wave_width, width, hidden, lens in CASES:
        for mode in ("sep", "inplace", "null"):
            staged, h_out, h_in = ask(exe, wave_width, width, hidden, mode, lens)
            want_staged, want_out = restated(wave_width, width, hidden, mode, lens)
            assert np.array_equal(staged, want_staged), (wave_width, width, mode)
            assert np.array_equal(h_out, want_out), (wave_width, width, mode)
            assert not np.any(h_out == SENTINEL)                    # every text got a state back
            if mode == "sep":
                assert np.array_equal(h_in, start_arrays(len(lens), width)[0])   # the caller's h_in is left alone


def test_the_header_is_plain_c_and_cxx_without_hip():
    for cc, lang in (("gcc", "c"), ("g++", "c++")):
        subprocess.run([cc, "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-I", CSRC, "-x", lang,
                        os.path.join(CSRC, "texts_states.h")], check=True)


def test_pack_and_unpack_are_inverse_through_the_plans_order(harness):
    check(harness)
    # what went through a wave came back to its own place: its own values plus the device's half, nobody else's
    for wave_width, width, hidden, lens in CASES[:3]:
        _, h_out, _ = ask(harness, wave_width, width, hidden, "sep", lens)
        h_in, _ = start_arrays(len(lens), width)
        for k, n in enumerate(lens):
            assert np.array_equal(h_out[k, 1:hidden + 1], h_in[k, 1:hidden + 1] + np.float32(0.5 if n >= 2 else 0.0))


def test_the_fallback_row_reaches_every_row_and_every_text_without_one(harness):
    for wave_width, width, hidden, lens in CASES:
        staged, h_out, _ = ask(harness, wave_width, width, hidden, "null", lens)
        fallback = start_arrays(len(lens), width)[1]
        assert np.all(staged[:, 1:hidden + 1] == fallback[1:hidden + 1]) and np.all(staged[:, 0] == 0)
        assert np.all(staged[:, hidden + 1:] == 0)
        for k, n in enumerate(lens):
            assert np.array_equal(h_out[k, 1:hidden + 1], fallback[1:hidden + 1] + np.float32(0.5 if n >= 2 else 0.0))


def test_an_update_in_place_is_the_update_into_another_array(harness):
    for wave_width, width, hidden, lens in CASES:
        _, apart, _ = ask(harness, wave_width, width, hidden, "sep", lens)
        _, h_out, h_in = ask(harness, wave_width, width, hidden, "inplace", lens)
        assert np.array_equal(h_out, h_in)                          # the same array
        assert np.array_equal(h_out[:, 1:hidden + 1], apart[:, 1:hidden + 1])


@pytest.mark.parametrize("broken", ["caller order as plan order", "wave offset dropped", "no-row fill skipped"])
def test_each_rule_of_the_permutation_is_noticed(harness, broken):
    """the restatement with one rule broken differs from the header on the first three cases, in every mode it can"""
    noticed = 0
    for wave_width, width, hidden, lens in CASES[:3]:
        for mode in ("sep", "inplace", "null"):
            staged, h_out, _ = ask(harness, wave_width, width, hidden, mode, lens)
            bad_staged, bad_out = restated(wave_width, width, hidden, mode, lens, broken)
            differs = not (np.array_equal(staged, bad_staged) and np.array_equal(h_out, bad_out))
            # (with h_in NULL every start state is the same row, so an order cannot show in it; in place a text without
            # a row already holds its start state where it carries one)
            if mode == "sep" or (mode == "inplace" and broken != "no-row fill skipped"):
                assert differs, (broken, wave_width, width, mode)
            noticed += differs
    assert noticed >= 6


def test_under_address_and_undefined_behaviour_sanitizers(sanitized):
    """stand-alone: the harness has its own main, the sanitizers' runtimes are linked into it.  Its staging buffer has
    exactly the wave's rows and its arrays exactly n_texts rows: a row too many is a finding"""
    check(sanitized)


# ---------------------------------------------------------------- through the library, without a device


@pytest.fixture(scope="module")
def lib():
    return rc.bind_char(rc.load_amd())


@pytest.fixture()
def nets(lib):
    net = lib.rnn_new(42, 39, 42, rc.FLAG_STANDARD, 1, None, 4, 1e-3, 0.9, 0.0, rc.RELU)
    bottom = lib.rnn_new_with_bottom_layer(42, 16, 39, 42, rc.FLAG_STANDARD, 5, None, 4, 1e-3, 0.9, 0.0, rc.RELU, 0)
    yield net, bottom
    lib.rnn_delete_net(bottom)
    lib.rnn_delete_net(net)


def states_for(net, n, seed=3):
    H = net.contents.h_size
    return np.random.default_rng(seed).standard_normal((n, H)).astype(np.float32)


def dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_run_and_trace_refusals_and_early_returns_need_no_device(lib, nets):
    net, bottom = nets
    H, hidden = net.contents.h_size, net.contents.hidden_size
    texts = [np.array([3, 4, 5], np.uint8), np.array([6], np.uint8), np.array([7, 8], np.uint8)]
    ptrs = (rc.c_u8_p * 3)(*[rc.u8ptr(t) for t in texts])
    lens = np.array([3, 1, 2], np.int32)
    h_in = states_for(net, 3)
    h_out = np.full((3, H), SENTINEL)
    sums = np.full(3 * 3, 7.0)
    logp = [np.full(8, np.nan, np.float32) for _ in texts]
    lpp = (rc.c_float_p * 3)(*[rc.fptr(a) for a in logp])

    def run(net=net, texts=ptrs, lens=rc.iptr(lens), n=3, alen=0, h_in=rc.fptr(h_in), h_out=rc.fptr(h_out), sums=dptr(sums)):
        return lib.rnn_amd_run_texts_from(net, texts, lens, None, n, alen, h_in, h_out, sums)

    def trace(net=net, texts=ptrs, lens=rc.iptr(lens), n=3, alen=0, h_in=rc.fptr(h_in), h_out=rc.fptr(h_out), logp=lpp):
        return lib.rnn_amd_trace_texts_from(net, texts, lens, n, alen, h_in, h_out, logp, None)

    def untouched():
        return np.all(h_out == SENTINEL) and np.all(sums == 7.0) and all(np.all(np.isnan(a)) for a in logp)

    kept = h_in.copy()
    # everything the counterparts refuse, with or without states
    for call in (run, trace):
        for states in ({}, {"h_in": None}, {"h_out": None}, {"h_in": None, "h_out": None}):
            assert call(net=None, **states) == -1 and call(net=bottom, **states) == -1 and call(n=-1, **states) == -1
            assert call(texts=None, **states) == -1 and call(lens=None, **states) == -1
            assert call(alen=5, **states) == -1 and call(alen=-14, **states) == -1     # 42 outputs are not heads of 5
            assert call(texts=(rc.c_u8_p * 3)(None, rc.u8ptr(texts[1]), rc.u8ptr(texts[2])), **states) == -1
    assert trace(logp=None) == -1 and trace(logp=None, h_in=None) == -1                # a trace needs its arrays ...
    assert trace(logp=(rc.c_float_p * 3)(None, None, None)) == -1
    assert run(sums=None, h_out=None) == -1 and run(sums=None, h_out=None, h_in=None) == -1   # ... the sums form sums or states
    assert untouched() and np.array_equal(h_in, kept)
    # n_texts == 0 returns 0 and touches nothing
    assert run(n=0) == 0 and run(n=0, texts=None, lens=None, h_in=None, h_out=None, sums=None) == 0
    assert trace(n=0) == 0 and trace(n=0, texts=None, lens=None, h_in=None, h_out=None, logp=None) == 0
    assert untouched()
    # every text shorter than 2 symbols and h_in given: h_out is h_in where a state carries information, by the host alone
    short = np.array([1, 0, 1], np.int32)
    for call in (run, trace):
        h_out[:] = SENTINEL
        assert call(lens=rc.iptr(short)) == 0
        assert np.array_equal(h_out[:, 1:hidden + 1], h_in[:, 1:hidden + 1]) and not np.any(np.isnan(h_out))
    assert np.all(sums[:3] == 0.0) and np.array_equal(h_in, kept)
    h_out[:] = SENTINEL
    assert run(lens=rc.iptr(short), sums=None) == 0                                     # the batched rnn_char_prime
    assert np.array_equal(h_out[:, 1:hidden + 1], h_in[:, 1:hidden + 1])
    # NaN in element 0 and in the padding of h_in is never read
    dirty = h_in.copy()
    dirty[:, 0] = np.nan
    dirty[:, hidden + 1:] = np.nan
    assert run(lens=rc.iptr(short), h_in=rc.fptr(dirty)) == 0
    assert np.array_equal(h_out[:, 1:hidden + 1], h_in[:, 1:hidden + 1])
    # in place
    same = h_in.copy()
    assert run(lens=rc.iptr(short), h_in=rc.fptr(same), h_out=rc.fptr(same)) == 0
    assert np.array_equal(same[:, 1:hidden + 1], h_in[:, 1:hidden + 1])
    # h_in NULL: the start state is the net's hidden row, which a fresh net holds on the host (zeros)
    h_out[:] = SENTINEL
    assert run(lens=rc.iptr(short), h_in=None) == 0
    row = rc.view(net.contents.hidden_layer, H)
    assert np.array_equal(h_out[:, 1:hidden + 1], np.tile(row[1:hidden + 1], (3, 1)))
    # the drivers on the same ground
    got, back = run_texts_from(lib, net, [t[:1] for t in texts], h_in=h_in)
    assert list(got) == [0.0] * 3 and np.array_equal(back[:, 1:hidden + 1], h_in[:, 1:hidden + 1])
    traced, back = trace_texts_from(lib, net, [t[:1] for t in texts], h_in=h_in)
    assert [a.shape for a, _ in traced] == [(0, 1)] * 3 and np.array_equal(back[:, 1:hidden + 1], h_in[:, 1:hidden + 1])
    got, back = run_texts_from(lib, net, [], h_in=np.zeros((0, H), np.float32))
    assert got.shape == (0,) and back.shape == (0, H)
    with pytest.raises(ValueError):
        run_texts_from(lib, bottom, [t[:1] for t in texts])


def test_continue_refusals_and_early_returns_need_no_device(lib, nets):
    net, bottom = nets
    H, hidden = net.contents.h_size, net.contents.hidden_size
    prompts = [np.array([3, 4, 5], np.uint8), np.array([6], np.uint8)]
    ptrs = (rc.c_u8_p * 2)(*[rc.u8ptr(t) for t in prompts])
    plens = np.array([3, 1], np.int32)
    seeds = np.array([11, 12], np.uint64)
    sp = seeds.ctypes.data_as(C.POINTER(C.c_uint64))
    rng_in = np.arange(1, 9, dtype=np.uint64).reshape(2, 4)
    gp = rng_in.ctypes.data_as(C.POINTER(rc.RandCtx))
    h_in = states_for(net, 2)
    h_out = np.full((2, H), SENTINEL)
    out = np.full((2, 10), 0xEE, np.uint8)
    lens = np.full(2, -7, np.int32)
    rng_out = np.full((2, 4), 99, np.uint64)
    gop = rng_out.ctypes.data_as(C.POINTER(rc.RandCtx))

    def call(net=net, prompts=ptrs, plens=rc.iptr(plens), seeds=sp, rng_in=None, n=2, max_len=10, alen=0, head=0,
             h_in=rc.fptr(h_in), h_out=rc.fptr(h_out), out=rc.u8ptr(out), lens=rc.iptr(lens), rng_out=gop):
        return lib.rnn_amd_continue_texts_from(net, prompts, plens, seeds, rng_in, n, max_len, 0.0, -1, alen, head, h_in, h_out,
                                               out, lens, rng_out)

    def untouched():
        return np.all(h_out == SENTINEL) and np.all(out == 0xEE) and np.all(lens == -7) and np.all(rng_out == 99)

    for states in ({}, {"h_in": None}, {"h_out": None}, {"h_in": None, "h_out": None}, {"rng_in": gp}, {"rng_in": gp, "seeds": None}):
        assert call(net=None, **states) == -1 and call(net=bottom, **states) == -1
        assert call(n=-1, **states) == -1 and call(max_len=-1, **states) == -1
        assert call(prompts=None, **states) == -1 and call(plens=None, **states) == -1
        assert call(out=None, **states) == -1 and call(lens=None, **states) == -1
        assert call(alen=5, **states) == -1 and call(alen=14, head=3, **states) == -1 and call(head=1, **states) == -1
        assert call(plens=rc.iptr(np.array([3, 0], np.int32)), **states) == -1
        assert call(prompts=(rc.c_u8_p * 2)(rc.u8ptr(prompts[0]), None), **states) == -1
        assert call(prompts=(rc.c_u8_p * 2)(rc.u8ptr(np.array([3, 42, 5], np.uint8)), rc.u8ptr(prompts[1])), **states) == -1
        assert call(plens=rc.iptr(np.array([3, 2 ** 31 - 5], np.int32)), **states) == -1
    assert call(seeds=None) == -1 and call(seeds=None, rng_in=None, h_in=None, h_out=None) == -1   # neither seeds nor generators
    assert untouched()
    # n_texts == 0 returns 0 and touches nothing
    assert call(n=0) == 0
    assert call(n=0, prompts=None, plens=None, seeds=None, h_in=None, h_out=None, out=None, lens=None, rng_out=None) == 0
    assert untouched()
    # max_len == 0: lengths zeroed, the start generator and the start state handed back, no device asked for
    assert call(max_len=0) == 0
    assert list(lens) == [0, 0] and np.all(out == 0xEE)
    assert np.array_equal(h_out[:, 1:hidden + 1], h_in[:, 1:hidden + 1])
    orc = rc.load_oracle()
    import sample_oracle as so
    assert [tuple(int(x) for x in g) for g in rng_out] == [so.words(so.seeded(orc, int(s))) for s in seeds]
    rng_out[:] = 99
    assert call(max_len=0, rng_in=gp, seeds=None) == 0 and np.array_equal(rng_out, rng_in)
    h_out[:] = SENTINEL
    assert call(max_len=0, h_in=None) == 0                       # the net's hidden row: a fresh net's is on the host
    row = rc.view(net.contents.hidden_layer, H)
    assert np.array_equal(h_out[:, 1:hidden + 1], np.tile(row[1:hidden + 1], (2, 1)))
    # the driver
    texts, gens, back = continue_texts_from(lib, net, prompts, None, 0, h_in=h_in, rng_in=rng_in)
    assert [len(t) for t in texts] == [0, 0] and np.array_equal(gens, rng_in)
    assert np.array_equal(back[:, 1:hidden + 1], h_in[:, 1:hidden + 1])


def test_the_character_layer_refuses_before_it_needs_a_device(lib, nets):
    net, bottom = nets
    alphabet = rc.default_text_alphabet(lib)
    prompts = (C.c_char_p * 2)(b"the cat", b"a dog")
    nbytes_in = np.array([7, 5], np.int32)
    seeds = np.arange(6, dtype=np.uint64)
    sp = seeds.ctypes.data_as(C.POINTER(C.c_uint64))
    bufs = [C.create_string_buffer(b"\x55" * 8, 8) for _ in range(6)]
    dest = (C.c_char_p * 6)(*[C.cast(b, C.c_char_p) for b in bufs])
    nbytes = np.full(6, -7, np.int32)
    ent = np.full(2, 7.0)

    def call(net=net, a=alphabet, prompts=prompts, pb=rc.iptr(nbytes_in), seeds=sp, n=2, repeats=3, chars=5, dest=dest,
             byte_len=8, nbytes=rc.iptr(nbytes), ent=dptr(ent)):
        return lib.rnn_amd_char_score_and_continue_texts(net, a, prompts, pb, seeds, n, repeats, chars, 0.0, -1, dest, byte_len,
                                                         nbytes, ent)

    assert call(net=None) == -1 and call(a=None) == -1 and call(n=-1) == -1 and call(chars=-1) == -1
    assert call(repeats=0) == -1 and call(repeats=-2) == -1 and call(repeats=2 ** 30) == -1
    assert call(prompts=None) == -1 and call(pb=None) == -1 and call(seeds=None) == -1 and call(dest=None) == -1
    assert call(nbytes=None) == -1 and call(ent=None) == -1
    assert np.all(nbytes == -7) and np.all(ent == 7.0) and all(b.raw == b"\x55" * 8 for b in bufs)
    assert call(n=0) == 0 and np.all(nbytes == -7)
    assert call(net=bottom) == -1                                   # rnn_amd_run_texts_from's refusal passes through
    assert np.all(ent == 7.0)
    assert call(prompts=(C.c_char_p * 2)(b"the cat", b"")) == -1    # a prompt that encodes to no symbol
    assert list(nbytes) == [0] * 6 and all(b.raw[0] == 0 for b in bufs)
    nbytes[:] = -7
    assert call(byte_len=1) == 0 and list(nbytes) == [0] * 6       # too little room writes nothing but the NUL
    lib.rnn_char_free_alphabet(alphabet)
