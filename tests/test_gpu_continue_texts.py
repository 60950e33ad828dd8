"""Many prompts continued by one net in one batched device run (rnn_amd_continue_texts, rnn_amd_char_continue_texts;
recur_amd/csrc/sample_api.c, continue_rule.h, k_texts_continue in kernels_rows.hip) against the oracle.

The comparison is TEACHER-FORCED, as tests/test_gpu_sample_texts.py's is and for its reason: oracle stream k starts from the
net's hidden row, is fed prompt[:-1] (sample_oracle.scores_of, the scores thrown away: rnn_char_prime's loop), and then
sample_oracle.replay follows the device's continuation from prompt[-1] with a generator seeded seeds[k].  The acceptance
conditions are that module's `checked`, unchanged: every pick allowed at TOL = 1e-4; picks that differ from the oracle's
strict pick at most max(1, 0.2 %) of the steps; steps within TOL of a boundary under 5 % of the steps -- a cap, not a
measurement: a u lies within 1e-4 of one of at most alen boundaries with probability at most 2e-4 * alen, 0.84 % for 42
symbols and 1.5 % for 73 --; a text with no close step equals the strict picks exactly and leaves the replayed generator,
all four words.  Every teacher-forced call has at least 300 drawn steps.

The nets are the `trained()` nets of test_gpu_run_texts.py, the hidden-1024 net is test_gpu_texts_wide.py's.  Prompts are
slices of the erewhon text, taken modulo the symbol count.  No test here feeds NaNs or aims at the draw's attempt cap:
tests/test_sample_rule.py covers it on the CPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import recur_ctypes as rc
import sample_oracle as so
from recur_amd.drivers import continue_texts, run_texts, sample_texts
from test_gpu_run_texts import erewhon, forward_clone, hidden_row, oracle_like, rng_of, trained

pytestmark = pytest.mark.gpu
SPACE = rc.DEFAULT_CHARSET.index(b" ")
RAGGED = [1, 2, 3, 17, 64, 65, 65, 2]  # an order that is not the plan's, equal lengths, one row past the look at step 64


@pytest.fixture(scope="module")
def amd():
    lib = rc.bind_char(rc.load_amd())
    assert lib.rnn_amd_device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return lib


def prompts_of(lens, symbols=None, at=30000, apart=97):
    text = erewhon(symbols)
    return [np.ascontiguousarray(text[at + apart * k:at + apart * k + n]) for k, n in enumerate(lens)]


def primed(o, k, prompt, alen, head=0):
    """oracle stream k fed all of the prompt but its last symbol"""
    for s in prompt[:-1]:
        so.scores_of(o, k, s, alen, head)


def checked(lib, a, net, prompts, seeds, max_len, bias, stop=-1, alphabet_len=0, head=0, what=""):
    """one batched call, then every continuation followed by the oracle: the conditions of the module's docstring"""
    texts, rngs = continue_texts(lib, net, prompts, seeds, max_len, bias, stop, alphabet_len, head)
    alen = alphabet_len or a.output_size
    o = oracle_like(lib, a, net, len(prompts))
    steps = differing = close = exact_rows = 0
    for k, t in enumerate(texts):
        assert 1 <= len(t) <= max_len and np.all(t < alen)
        assert (len(t) == max_len or t[-1] == stop) and not np.any(t[:-1] == stop)
        primed(o, k, prompts[k], alen, head)
        r = so.replay(o, k, prompts[k][-1], seeds[k], t, bias, alen, head)
        steps += len(t)
        differing += r.differing(t)
        close += len(r.close)
        if not r.close:
            exact_rows += 1
            assert list(t) == r.strict, (k, list(t), r.strict)
            assert tuple(int(x) for x in rngs[k]) == r.rng, k
        if bias >= so.GREEDY_BIAS:
            assert tuple(int(x) for x in rngs[k]) == so.words(so.seeded(o.orc, seeds[k]))  # no draw: untouched
    o.close()
    print("%s: %d prompts, %d steps, %d picks differ from the oracle's strict pick, %d steps within %g of a boundary (%.2f %%), "
          "%d texts compared exactly" % (what, len(texts), steps, differing, close, so.TOL, 100.0 * close / steps, exact_rows))
    assert steps >= 300  # (of the test's design, not of the library: the 5 % below is not a matter of luck)
    assert differing <= max(1, 0.002 * steps)
    assert close < 0.05 * steps
    return texts, rngs


def same(one, two):
    (t1, r1), (t2, r2) = one, two
    return len(t1) == len(t2) and all(np.array_equal(x, y) for x, y in zip(t1, t2)) and np.array_equal(r1, r2)


def test_one_symbol_prompts_are_the_sampler_bit_for_bit(amd):
    a = trained(amd)
    net = forward_clone(amd, a.net)
    first = [3 + 2 * k for k in range(8)]
    seeds = [100 + k for k in range(8)]
    prompts = [np.array([f], np.uint8) for f in first]
    for bias in (0.0, 1.0, 200.0):
        assert same(continue_texts(amd, net, prompts, seeds, 40, bias), sample_texts(amd, net, first, seeds, 40, bias)), bias
    assert same(continue_texts(amd, net, prompts, seeds, 40, 0.0, stop=SPACE),
                sample_texts(amd, net, first, seeds, 40, 0.0, stop=SPACE))
    amd.rnn_delete_net(net)
    # two waves, the second narrower
    a = trained(amd, hidden=39)
    net = forward_clone(amd, a.net)
    first = [k % 42 for k in range(300)]
    seeds = [7000 + 13 * k for k in range(300)]
    got = continue_texts(amd, net, [np.array([f], np.uint8) for f in first], seeds, 12)
    assert same(got, sample_texts(amd, net, first, seeds, 12))
    assert len({t.tobytes() for t in got[0]}) > 250
    amd.rnn_delete_net(net)


@pytest.mark.parametrize("hidden,symbols", [(39, 42), (99, 42), (130, 73), (256, 42)])
def test_ragged_prompts(amd, hidden, symbols):
    a = trained(amd, hidden=hidden, symbols=symbols)
    net = forward_clone(amd, a.net)
    prompts = prompts_of(RAGGED, symbols)
    seeds = [100 + k for k in range(8)]
    what = "hidden %d, %d symbols, " % (hidden, symbols)
    plain, _ = checked(amd, a, net, prompts, seeds, 40, 0.0, what=what + "bias 0")
    sharp, _ = checked(amd, a, net, prompts, seeds, 40, 1.0, what=what + "bias 1")
    assert len({t.tobytes() for t in plain}) == 8          # eight generators, eight texts
    assert any(not np.array_equal(x, y) for x, y in zip(plain, sharp))
    if hidden == 99:
        checked(amd, a, net, prompts, seeds, 40, 200.0, what=what + "greedy")
    amd.rnn_delete_net(net)


def test_the_callers_order_does_not_matter(amd):
    a = trained(amd)
    net = forward_clone(amd, a.net)
    lens = [5, 9, 1, 30, 12, 2, 70, 3]  # no ties: the same plan, row for row, whatever the caller's order
    prompts = prompts_of(lens)
    seeds = [40 + k for k in range(8)]
    texts, rngs = continue_texts(amd, net, prompts, seeds, 30, 0.0)
    back, brngs = continue_texts(amd, net, prompts[::-1], seeds[::-1], 30, 0.0)
    assert same((texts, rngs), (back[::-1], brngs[::-1]))
    assert len({t.tobytes() for t in texts}) == 8
    amd.rnn_delete_net(net)


def seeds_that_stop_early(lib, a, net, prompts, before, bias=0.0):
    """on the oracle alone: for every prompt the first seed whose continuation meets the space symbol before step
    `before`, no step of it within TOL of a boundary"""
    o = oracle_like(lib, a, net, 1)
    start = o.arrays()["hidden"].copy()
    seeds = []
    for p in prompts:
        o.arrays()["hidden"][:] = start
        primed(o, 0, p, a.output_size)
        after_prompt = o.arrays()["hidden"].copy()
        for seed in range(500, 700):
            o.arrays()["hidden"][:] = after_prompt
            t, close, _ = so.free_run(o, 0, p[-1], seed, before, bias, stop=SPACE)
            if t[-1] == SPACE and not close:
                seeds.append(seed)
                break
    o.close()
    assert len(seeds) == len(prompts)
    return seeds


def test_a_stop_symbol(amd):
    lib = amd
    a = trained(lib)
    net = forward_clone(lib, a.net)
    n, max_len = 128, 30
    prompts = prompts_of([1 + (7 * k) % 23 for k in range(n)], apart=41)
    assert sum(SPACE in p for p in prompts) > n // 2 and sum(p[-1] == SPACE for p in prompts) >= 4  # (ended by none)
    seeds = seeds_that_stop_early(lib, a, net, prompts[:4], 20) + [900 + k for k in range(4, n)]
    texts, _ = checked(lib, a, net, prompts, seeds, max_len, 0.0, stop=SPACE, what="until a drawn space")
    lens = [len(t) for t in texts]
    print("lengths", lens)
    assert all(len(t) <= 20 and t[-1] == SPACE for t in texts[:4])
    assert len(set(lens)) > 3  # (continue_texts has checked that nothing lies behind a text's length)
    lib.rnn_delete_net(net)


@pytest.mark.parametrize("kind", ["training", "forward"])
def test_the_start_state_is_taken_and_the_net_left_alone(amd, kind):
    lib = amd
    a = trained(lib)
    net = a.nets[0] if kind == "training" else forward_clone(lib, a.net)
    prompts = prompts_of(RAGGED)
    seeds = [60 + k for k in range(8)]
    unprimed, _ = continue_texts(lib, net, prompts, seeds, 40)
    prefix = np.ascontiguousarray(erewhon()[29000:29100])
    assert lib.rnn_char_prime(net, None, rc.u8ptr(prefix), len(prefix)) == int(prefix[-1])
    fixed = [np.ascontiguousarray(erewhon()[31000:31120])]
    hid, rng, score = hidden_row(lib, net), rng_of(lib, net), run_texts(lib, net, fixed)[0]
    texts, _ = checked(lib, a, net, prompts, seeds, 40, 0.0, what="primed " + kind)
    short = [0, 1, 2, 7]  # prompts of up to 3 symbols: the state they start from is not forgotten
    assert sum(not np.array_equal(texts[k], unprimed[k]) for k in short) >= 3  # the same generators, another state
    # the net is where it was: hidden row bit for bit, generator, and what it computes next
    assert np.array_equal(hidden_row(lib, net), hid) and rng_of(lib, net) == rng
    again = run_texts(lib, net, fixed)[0]
    print("the fixed text before", score, "and after", again)
    assert again == score and score < 0.0
    if kind == "forward":
        lib.rnn_delete_net(net)


def test_heads(amd):
    """an output row of 3 heads of 14 symbols: the continuation drawn from head 1, and from head 2"""
    lib = amd
    a = trained(lib, hidden=99, symbols=42, text_symbols=14)
    net = forward_clone(lib, a.net)
    prompts = prompts_of(RAGGED, 14)
    seeds = [300 + k for k in range(8)]
    one, _ = checked(lib, a, net, prompts, seeds, 40, 0.0, alphabet_len=14, head=1, what="head 1 of 3")
    two, _ = checked(lib, a, net, prompts, seeds, 40, 0.0, alphabet_len=14, head=2, what="head 2 of 3")
    assert sum(not np.array_equal(x, y) for x, y in zip(one, two)) >= 6
    lib.rnn_delete_net(net)


def test_hidden_1024(amd):
    from test_gpu_texts_wide import a_clone, wide
    w = wide(amd, "A")
    net = a_clone(amd, w)
    prompts = prompts_of(range(1, 9))
    checked(amd, w, net, prompts, [1 + k for k in range(8)], 40, 0.0, what="A 42/1024/42")
    amd.rnn_delete_net(net)


def char_continue_texts(lib, net, alphabet, prompts, seeds, char_len, bias, stop, byte_len):
    n = len(seeds)
    bufs = [C.create_string_buffer(max(byte_len, 1)) for _ in range(n)]
    dest = (C.c_char_p * n)(*[C.cast(b, C.c_char_p) for b in bufs])
    ps = (C.c_char_p * n)(*prompts)
    pb = np.array([len(p) for p in prompts], np.int32)
    sd = np.ascontiguousarray(seeds, np.uint64)
    nbytes = np.full(n, -1, np.int32)
    r = lib.rnn_amd_char_continue_texts(net, alphabet, ps, rc.iptr(pb), sd.ctypes.data_as(C.POINTER(C.c_uint64)), n, char_len,
                                        bias, stop, dest, byte_len, rc.iptr(nbytes))
    return r, [b.value for b in bufs], list(nbytes)


def encoded(lib, alphabet, raw):
    n = C.c_int(0)
    p = lib.rnn_char_alloc_encoded_text(alphabet, raw, len(raw), C.byref(n), None, False)
    return np.ctypeslib.as_array(p, shape=(n.value,)).copy()


def decoded(alphabet, syms, byte_len, utf8):
    """the room rule of rnn_char_confabulate: symbols are written while fewer than byte_len - (utf8 ? 5 : 1) bytes are used"""
    room, out = byte_len - (5 if utf8 else 1), b""
    for s in syms:
        if len(out) >= room:
            break
        point = alphabet.contents.points[int(s)]
        out += chr(point).encode("utf-8") if utf8 else bytes([point])
    return out


def test_the_char_layer_is_encode_continue_decode(amd):
    lib = amd
    a = trained(lib)
    net = forward_clone(lib, a.net)
    seeds = [21, 22, 23, 24]
    # text-predict's alphabet: bytes, case folded, spaces collapsed
    alphabet = rc.default_text_alphabet(lib)
    raw = [b"The  higher Alps", b"a", b"and  WHAT then?", b"  x"]
    prompts = [encoded(lib, alphabet, p) for p in raw]
    assert [len(p) for p in prompts] == [15, 1, 14, 1]          # (spaces collapsed, also in front)
    for bias, stop, byte_len in ((0.0, -1, 400), (1.0, SPACE, 400), (0.0, -1, 8)):
        syms, _ = continue_texts(lib, net, prompts, seeds, 40, bias, stop)
        r, got, nbytes = char_continue_texts(lib, net, alphabet, raw, seeds, 40, bias, stop, byte_len)
        assert r == 0 and got == [decoded(alphabet, s, byte_len, False) for s in syms] and nbytes == [len(g) for g in got]
        assert all(len(g) == (7 if byte_len == 8 else len(s)) for g, s in zip(got, syms))
    r, got, nbytes = char_continue_texts(lib, net, alphabet, raw, seeds, 40, 0.0, -1, 1)   # no room: nothing but the NUL
    assert r == 0 and got == [b""] * 4 and nbytes == [0] * 4
    r, got, nbytes = char_continue_texts(lib, net, alphabet, [b"the", b"", b"a", b"b"], seeds, 40, 0.0, -1, 400)
    assert r == -1 and got == [b""] * 4 and nbytes == [0] * 4                             # a prompt without a symbol
    lib.rnn_char_free_alphabet(alphabet)
    # a utf-8 alphabet on the same net: the symbols the net likes best take 2, 3 and 4 bytes
    points = list(rc.DEFAULT_CHARSET)
    for sym, point in ((2, 0xE9), (3, 0x20AC), (5, 0x1F600), (4, 0x101)):
        points[sym] = point
    alphabet = lib.rnn_char_new_alphabet()
    lib.rnn_char_alphabet_set_flags(alphabet, False, True, False)
    for i, p in enumerate(points):
        alphabet.contents.points[i] = p
    alphabet.contents.len = len(points)
    raw = ["hé €ā  n".encode("utf-8"), "\U0001F600".encode("utf-8"), b"no such: TEXT", "āā".encode("utf-8")]
    prompts = [encoded(lib, alphabet, p) for p in raw]
    assert [len(p) for p in prompts] == [8, 1, 13, 2] and list(prompts[1]) == [5]          # code points, spaces kept
    for byte_len in (400, 23):
        syms, _ = continue_texts(lib, net, prompts, seeds, 40, 1.0)
        r, got, nbytes = char_continue_texts(lib, net, alphabet, raw, seeds, 40, 1.0, -1, byte_len)
        assert r == 0 and got == [decoded(alphabet, s, byte_len, True) for s in syms] and nbytes == [len(g) for g in got]
        assert all(len(g) >= 40 for g in got) if byte_len == 400 else all(18 <= len(g) <= 21 for g in got)
        assert all(g.decode("utf-8") for g in got)                                         # whole code points
    lib.rnn_char_free_alphabet(alphabet)
    lib.rnn_delete_net(net)


def test_the_tool_continues_the_lines_of_a_file(amd, tmp_path):
    lib = amd
    build = os.path.join(rc.ROOT, "build")
    path = str(tmp_path / "erewhon.net")
    r = subprocess.run([os.path.join(build, "text_predict_amd"), "-f", rc.EREWHON, "-H", "99", "-t", "16", "-d", "10",
                        "-l", "1e-3", "-s", "60", "-r", "60", "-V", "1500", "-n", path],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0 and os.path.exists(path), r.stderr[-2000:]
    lines = ["the higher", "It was a Long", "of"]
    with open(tmp_path / "prompts.txt", "w") as f:
        f.write(lines[0] + "\n\n" + lines[1] + "\r\n" + lines[2])   # an empty line, a CR, no newline at the end
    tool = [os.path.join(build, "text_confabulate_amd"), "-f", path, "-n", "30", "-B", "1", "-P", str(tmp_path / "prompts.txt")]

    def run(args, code=0):
        r = subprocess.run(tool + args, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert r.returncode == code, r.stderr[-2000:]
        return r.stdout.split("\n"), r.stderr

    out, _ = run(["-N", "2", "-r", "5"])
    assert len(out) == 7 and out[6] == ""
    rows = [lines[i // 2] for i in range(6)]
    assert all(o.startswith(p) and len(o) == len(p) + 30 for o, p in zip(out, rows))
    assert run(["-N", "2", "-r", "5"])[0] == out and run(["-N", "2", "-r", "6"])[0] != out   # deterministic for a seed
    # line i is the library's continuation with seed 5 + i
    net = lib.rnn_load_net(path.encode())
    alphabet = lib.rnn_char_new_alphabet_from_net(net)
    r, want, _ = char_continue_texts(lib, net, alphabet, [p.encode() for p in rows], [5 + i for i in range(6)], 30, 1.0, -1,
                                     30 * 4 + 5)
    assert r == 0 and [o[len(p):].encode() for o, p in zip(out, rows)] == want and len(set(want)) >= 5
    lib.rnn_char_free_alphabet(alphabet)
    lib.rnn_delete_net(net)
    # without -N: one continuation per line
    out1, _ = run(["-r", "5"])
    assert len(out1) == 4 and all(o.startswith(p) for o, p in zip(out1, lines))
    # -w does not go with -P
    out, err = run(["-w", "t"], code=2)
    assert "usage" in err and out == [""]
