"""Many texts drawn from one net in one batched device run (rnn_amd_sample_texts, rnn_amd_char_confabulate_texts;
recur_amd/csrc/sample_api.c, sample_rule.h, k_texts_continue in kernels_rows.hip) against the oracle.

A sampler is discontinuous: a probability that differs in its last bit can move one draw, and every symbol after it.  So
the comparison is TEACHER-FORCED (tests/sample_oracle.py, replay): for text k an oracle stream starts from the net's hidden
row with a generator seeded seeds[k], is fed at every step the symbol the DEVICE chose, computes its own distribution and
cumulative sums c, draws its own u (again, as the rule says, when u is not below the total), and accepts the device's pick
s when c[s - 1] - TOL <= u < c[s] + TOL.  TOL = 1e-4 is the project's parity bar on a quantity that is at most 1 (the
outputs themselves drift by about 3e-7).  On top of that, per test:
  * picks that differ from the oracle's strict pick (the first i with u < c[i]): at most max(1, 0.2 %) of the steps;
  * steps whose u lies within TOL of a boundary, by the oracle's own numbers: under 5 % (printed) -- the tolerance is not
    what makes the test pass;
  * a text with no such step equals the oracle's strict picks exactly, and its generator afterwards is the replayed
    generator, all four words.
With bias >= 100 there is no draw: the device's pick must be a best output of the oracle's (within TOL of the scores'
size), the strict pick is the last of equal maxima, and the generators are what they were seeded to.

The nets are the `trained()` nets of test_gpu_run_texts.py (erewhon, 60 generations), shared with that module.  No test
here feeds NaNs or otherwise aims at the draw's attempt cap: tests/test_sample_rule.py covers it on the CPU.  Their shapes
keep every forward pass on output=rows (k_out_layer; fwd_plan.h) and the head at 2 of 3 at most: the other output-layer
forms, a head far into a wide row and hidden 1024 are tests/test_gpu_texts_wide.py's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import recur_ctypes as rc
import sample_oracle as so
from recur_amd.drivers import sample_texts
from test_gpu_run_texts import erewhon, forward_clone, hidden_row, oracle_like, rng_of, trained

pytestmark = pytest.mark.gpu
SPACE = rc.DEFAULT_CHARSET.index(b" ")


@pytest.fixture(scope="module")
def amd():
    lib = rc.bind_char(rc.load_amd())
    assert lib.rnn_amd_device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return lib


def checked(lib, a, net, first, seeds, max_len, bias, stop=-1, alphabet_len=0, head=0, what="", before_step=None):
    """one batched call, then every text followed by the oracle: the conditions of the module's docstring"""
    texts, rngs = sample_texts(lib, net, first, seeds, max_len, bias, stop, alphabet_len, head)
    alen = alphabet_len or a.output_size
    o = oracle_like(lib, a, net, len(first))
    steps = differing = close = exact_rows = 0
    for k, t in enumerate(texts):
        assert 1 <= len(t) <= max_len and np.all(t < alen)
        assert (len(t) == max_len or t[-1] == stop) and not np.any(t[:-1] == stop)
        r = so.replay(o, k, first[k], seeds[k], t, bias, alen, head,
                      before_step=(lambda step, k=k: before_step(o, k, step)) if before_step else None)
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
    print("%s: %d texts, %d steps, %d picks differ from the oracle's strict pick, %d steps within %g of a boundary (%.2f %%), "
          "%d texts compared exactly" % (what, len(texts), steps, differing, close, so.TOL, 100.0 * close / steps, exact_rows))
    assert differing <= max(1, 0.002 * steps)
    assert close < 0.05 * steps
    return texts, rngs


@pytest.mark.parametrize("hidden,symbols", [(39, 42), (99, 42), (130, 73), (256, 42)])
def test_shapes(amd, hidden, symbols):
    a = trained(amd, hidden=hidden, symbols=symbols)
    net = forward_clone(amd, a.net)
    first = [3 + 2 * k for k in range(8)]
    seeds = [100 + k for k in range(8)]
    plain, _ = checked(amd, a, net, first, seeds, 40, 0.0, what="hidden %d, %d symbols, bias 0" % (hidden, symbols))
    sharp, _ = checked(amd, a, net, first, seeds, 40, 1.0, what="hidden %d, %d symbols, bias 1" % (hidden, symbols))
    best, _ = checked(amd, a, net, first, seeds, 40, 200.0, what="hidden %d, %d symbols, greedy" % (hidden, symbols))
    assert len({t.tobytes() for t in plain}) == 8          # eight generators, eight texts
    assert any(not np.array_equal(x, y) for x, y in zip(plain, sharp))
    amd.rnn_delete_net(net)


def test_two_waves_the_second_narrower(amd):
    a = trained(amd, hidden=39)
    net = forward_clone(amd, a.net)
    first = [k % 42 for k in range(300)]
    seeds = [7000 + 13 * k for k in range(300)]
    texts, _ = checked(amd, a, net, first, seeds, 12, 0.0, what="300 texts")
    # the rows of the second wave are their own: the texts of rows 256 ... alone are what they were in the batch
    again, _ = sample_texts(amd, net, first[256:], seeds[256:], 12)
    assert all(np.array_equal(x, y) for x, y in zip(again, texts[256:]))
    amd.rnn_delete_net(net)


def test_heads(amd):
    """an output row of 3 heads of 14 symbols: head 1 against the oracle's softmax over that slice"""
    lib = amd
    a = trained(lib, hidden=99, symbols=42, text_symbols=14)
    net = forward_clone(lib, a.net)
    first, seeds = [k % 14 for k in range(8)], [300 + k for k in range(8)]
    for bias in (0.0, 1.0):
        checked(lib, a, net, first, seeds, 40, bias, alphabet_len=14, head=1, what="head 1 of 3, bias %g" % bias)
    checked(lib, a, net, first, seeds, 40, 0.0, alphabet_len=14, head=2, what="head 2 of 3")
    # one head as wide as the row is the plain call, bit for bit
    whole, wrng = sample_texts(lib, net, first, seeds, 40, 0.0, alphabet_len=42, head=0)
    plain, prng = sample_texts(lib, net, first, seeds, 40, 0.0)
    assert all(np.array_equal(x, y) for x, y in zip(whole, plain)) and np.array_equal(wrng, prng)
    lib.rnn_delete_net(net)


def seeds_that_stop_early(lib, a, net, first, n, before, bias=0.0):
    """on the oracle alone: the first n seeds whose text from `first` meets the space symbol before step `before`, no
    step of it within TOL of a boundary"""
    o = oracle_like(lib, a, net, 1)
    start = o.arrays()["hidden"].copy()
    seeds = []
    for seed in range(500, 700):
        o.arrays()["hidden"][:] = start
        t, close, _ = so.free_run(o, 0, first, seed, before, bias, stop=SPACE)
        if t[-1] == SPACE and not close:
            seeds.append(seed)
        if len(seeds) == n:
            break
    o.close()
    assert len(seeds) == n
    return seeds


def test_a_stop_symbol(amd):
    lib = amd
    a = trained(lib)
    net = forward_clone(lib, a.net)
    first = [3] * 16
    texts, _ = checked(lib, a, net, first, [900 + k for k in range(16)], 30, 0.0, stop=SPACE, what="until a space")
    lens = [len(t) for t in texts]
    print("lengths", lens)
    assert len(set(lens)) > 3 and min(lens) < 30  # (sample_texts has checked that nothing lies behind a text's length)
    # every row done before the first look at the done words, at step 64: the early end of the wave changes nothing
    seeds = seeds_that_stop_early(lib, a, net, 3, 8, 40)
    short, srng = checked(lib, a, net, first[:8], seeds, 70, 0.0, stop=SPACE, what="max_len 70")
    assert max(len(t) for t in short) < 64 and all(t[-1] == SPACE for t in short)
    longer, lrng = sample_texts(lib, net, first[:8], seeds, 200, 0.0, stop=SPACE)
    assert all(np.array_equal(x, y) for x, y in zip(short, longer)) and np.array_equal(srng, lrng)
    lib.rnn_delete_net(net)


@pytest.mark.parametrize("kind", ["training", "forward"])
def test_the_start_state_is_taken_and_left_alone(amd, kind):
    lib = amd
    a = trained(lib)
    if kind == "training":
        net, twin = a.nets[0], a.nets[1]
    else:
        net, twin = forward_clone(lib, a.net), forward_clone(lib, a.net)
    lib.rnn_amd_sync_host(twin, rc.RNN_AMD_STREAM)
    rc.view(twin.contents.hidden_layer, a.H)[:] = hidden_row(lib, net)
    lib.rnn_amd_host_written(twin, rc.RNN_AMD_STREAM)
    first, seeds = [3] * 8, [40 + k for k in range(8)]
    unprimed, _ = sample_texts(lib, net, first, seeds, 30)
    prefix = np.ascontiguousarray(erewhon()[29000:29100])
    for x in (net, twin):
        assert lib.rnn_char_prime(x, None, rc.u8ptr(prefix), len(prefix)) == int(prefix[-1])
    hid, rng = hidden_row(lib, net), rng_of(lib, net)
    assert np.array_equal(hid, hidden_row(lib, twin))
    primed, _ = checked(lib, a, net, first, seeds, 30, 0.0, what="primed " + kind)
    assert sum(not np.array_equal(x, y) for x, y in zip(primed, unprimed)) >= 6  # the same generators, another state
    # the net is where it was: hidden row bit for bit, generator, and what it computes next
    assert np.array_equal(hidden_row(lib, net), hid) and rng_of(lib, net) == rng
    seg = np.ascontiguousarray(erewhon()[31000:31120])
    mine = lib.rnn_char_cross_entropy(net, None, rc.u8ptr(seg), len(seg), 3, None, 0)
    twins = lib.rnn_char_cross_entropy(twin, None, rc.u8ptr(seg), len(seg), 3, None, 0)
    print("after the batch", mine, "a twin that never saw it", twins)
    assert mine == twins
    if kind == "forward":
        lib.rnn_delete_net(twin)
        lib.rnn_delete_net(net)


def test_the_same_call_twice_gives_the_same_bytes(amd):
    a = trained(amd, hidden=130, symbols=73)
    net = forward_clone(amd, a.net)
    first, seeds = list(range(20)), [2 ** 40 + k for k in range(20)]
    one, rng1 = sample_texts(amd, net, first, seeds, 50, 1.0)
    two, rng2 = sample_texts(amd, net, first, seeds, 50, 1.0)
    assert all(np.array_equal(x, y) for x, y in zip(one, two)) and np.array_equal(rng1, rng2)
    amd.rnn_delete_net(net)


def test_the_soft_clip_in_the_feed_half(amd):
    """The doubled-weights net of test_gpu_run_texts.py's soft-clip test: the hidden values grow from symbol to symbol
    until an input row sums to more than 16 per element and maybe_scale_inputs (recur-nn.c:68-81) scales it, and the
    scores leave the softmax's [-60, 50] window.  Checked on the oracle while it follows the device: the clip fires in
    every text."""
    lib = amd
    a = trained(lib)
    n = a.net.contents
    a.sync()
    ih = rc.view(n.ih_weights, a.I, a.H)
    kept = ih.copy()
    ih *= np.float32(2.0)
    lib.rnn_amd_host_written(a.net, rc.RNN_AMD_WEIGHTS)
    try:
        net = forward_clone(lib, a.net)  # hidden row zero
        first = [int(erewhon()[at]) for at in (30290, 32088, 32581, 33741, 33683)]
        fired = {k: [] for k in range(5)}

        def row_sum(o, k, step):
            # the row rnn_opinion is about to build: bias, hidden values, one symbol (recur-nn.c:104-112)
            total = 1.0 + float(o.arrays()["hidden"][k][1:a.hidden_size + 1].astype(np.float64).sum()) + 1.0
            if total > a.I * 16:
                fired[k].append(step)

        checked(lib, a, net, first, [50 + k for k in range(5)], 12, 0.0, what="soft clip", before_step=row_sum)
        print("clipped steps", fired)
        assert all(fired[k] for k in range(5))
        lib.rnn_delete_net(net)
    finally:
        lib.rnn_amd_sync_host(a.net, rc.RNN_AMD_WEIGHTS)
        ih[:] = kept
        lib.rnn_amd_host_written(a.net, rc.RNN_AMD_WEIGHTS)


def confabulate_texts(lib, net, alphabet, seeds, char_len, bias, prev, stop, byte_len):
    n = len(seeds)
    bufs = [C.create_string_buffer(max(byte_len, 1)) for _ in range(n)]
    dest = (C.c_char_p * n)(*[C.cast(b, C.c_char_p) for b in bufs])
    sd = np.ascontiguousarray(seeds, np.uint64)
    nbytes = np.full(n, -1, np.int32)
    r = lib.rnn_amd_char_confabulate_texts(net, alphabet, sd.ctypes.data_as(C.POINTER(C.c_uint64)), n, char_len, bias, prev,
                                           stop, dest, byte_len, rc.iptr(nbytes))
    return r, [b.value for b in bufs], list(nbytes)


def clean_seeds(lib, a, net, first, n, max_len, bias):
    """on the oracle alone: the first n seeds whose text has no step within TOL of a boundary"""
    o = oracle_like(lib, a, net, 1)
    start = o.arrays()["hidden"].copy()
    seeds = []
    for seed in range(1, 200):
        o.arrays()["hidden"][:] = start
        if not so.free_run(o, 0, first, seed, max_len, bias)[1]:
            seeds.append(seed)
        if len(seeds) == n:
            break
    o.close()
    assert len(seeds) == n
    return seeds


def test_the_char_layer_is_rnn_char_confabulate_on_fresh_clones(amd):
    lib = amd
    a = trained(lib)
    alphabet = rc.default_text_alphabet(lib)
    net = forward_clone(lib, a.net)
    prefix = np.ascontiguousarray(erewhon()[29000:29040])
    prev = lib.rnn_char_prime(net, None, rc.u8ptr(prefix), len(prefix))
    hid = hidden_row(lib, net)
    orc = rc.load_oracle()
    for bias in (0.0, 1.0):
        seeds = clean_seeds(lib, a, net, prev, 6, 40, bias)
        r, got, nbytes = confabulate_texts(lib, net, alphabet, seeds, 40, bias, prev, -1, 400)
        assert r == 0 and nbytes == [len(g) for g in got] == [40] * 6
        # where the oracle, following the batch's symbols, first comes within TOL of a boundary
        o = oracle_like(lib, a, net, 6)
        compared = 0
        for k, seed in enumerate(seeds):
            syms = np.array([rc.DEFAULT_CHARSET.index(bytes([c])) for c in got[k]], np.uint8)
            rep = so.replay(o, k, prev, seed, syms, bias)
            upto = rep.close[0] if rep.close else 40
            clone = forward_clone(lib, a.net)
            lib.rnn_amd_sync_host(clone, rc.RNN_AMD_STREAM)
            rc.view(clone.contents.hidden_layer, a.H)[:] = hid
            g = so.seeded(orc, seed)
            clone.contents.rng.a, clone.contents.rng.b, clone.contents.rng.c, clone.contents.rng.d = so.words(g)
            lib.rnn_amd_host_written(clone, rc.RNN_AMD_STREAM)
            buf = C.create_string_buffer(400)
            wrote = lib.rnn_char_confabulate(clone, buf, 40, 400, alphabet, bias, C.byref(C.c_int(prev)), -1, -1)
            lib.rnn_delete_net(clone)
            assert wrote == 40 and buf.value[:upto] == got[k][:upto], (k, buf.value, got[k], upto)
            compared += upto
        o.close()
        print("bias %g: %d of %d steps compared byte for byte" % (bias, compared, 6 * 40))
        assert compared >= 0.75 * 6 * 40
    # a stop symbol ends the text behind it, as it ends rnn_char_confabulate's
    r, got, nbytes = confabulate_texts(lib, net, alphabet, [11, 12, 13, 14], 60, 0.0, prev, SPACE, 400)
    assert r == 0 and all(g.endswith(b" ") and g.count(b" ") == 1 or len(g) == 60 for g in got)
    # too little room: nothing is written
    r, got, nbytes = confabulate_texts(lib, net, alphabet, [1, 2, 3], 10, 1.0, prev, -1, 1)
    assert r == 0 and got == [b""] * 3 and nbytes == [0, 0, 0]
    # room for 7 bytes and the NUL
    r, got, nbytes = confabulate_texts(lib, net, alphabet, [1, 2, 3], 10, 1.0, prev, -1, 8)
    assert r == 0 and nbytes == [7, 7, 7] and all(len(g) == 7 for g in got)
    lib.rnn_char_free_alphabet(alphabet)
    lib.rnn_delete_net(net)


def test_the_tool_draws_passages_with_N_and_is_as_before_without(amd, tmp_path):
    lib = amd
    build = os.path.join(rc.ROOT, "build")
    path = str(tmp_path / "erewhon.net")
    r = subprocess.run([os.path.join(build, "text_predict_amd"), "-f", rc.EREWHON, "-H", "99", "-t", "16", "-d", "10",
                        "-l", "1e-3", "-s", "60", "-r", "60", "-V", "1500", "-n", path],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0 and os.path.exists(path), r.stderr[-2000:]
    tool = [os.path.join(build, "text_confabulate_amd"), "-f", path, "-n", "30", "-p", "the ", "-B", "1"]

    def lines(args, code=0):
        r = subprocess.run(tool + args, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert r.returncode == code, r.stderr[-2000:]
        return r.stdout.split("\n"), r.stderr

    def primed(seed):
        """what the tool does before it draws: load, seed the net's generator, prime with the prefix"""
        net = lib.rnn_load_net(path.encode())
        alphabet = lib.rnn_char_new_alphabet_from_net(net)
        g = so.seeded(rc.load_oracle(), seed)
        net.contents.rng.a, net.contents.rng.b, net.contents.rng.c, net.contents.rng.d = so.words(g)
        lib.rnn_amd_host_written(net, rc.RNN_AMD_STREAM)
        n = C.c_int(0)
        p = lib.rnn_char_alloc_encoded_text(alphabet, b"the ", 4, C.byref(n), None, False)
        prefix = np.ctypeslib.as_array(p, shape=(n.value,)).copy()
        return net, alphabet, lib.rnn_char_prime(net, alphabet, rc.u8ptr(prefix), len(prefix))

    # -N 3 -r 5: three lines, line i the library's passage with seed 5 + i
    out, _ = lines(["-N", "3", "-r", "5"])
    assert len(out) == 4 and out[3] == ""
    net, alphabet, prev = primed(5)
    r, want, _ = confabulate_texts(lib, net, alphabet, [5, 6, 7], 30, 1.0, prev, -1, 30 * 4 + 5)
    assert r == 0 and [x.encode() for x in out[:3]] == want and len(set(want)) == 3
    lib.rnn_char_free_alphabet(alphabet)
    lib.rnn_delete_net(net)
    # without -N: one passage with the net's own generator, seeded by -r, as before
    net, alphabet, prev = primed(5)
    buf = C.create_string_buffer(30 * 4 + 5)
    lib.rnn_char_confabulate(net, buf, 30, 30 * 4 + 5, alphabet, 1.0, C.byref(C.c_int(prev)), -1, -1)
    lib.rnn_char_free_alphabet(alphabet)
    lib.rnn_delete_net(net)
    out, _ = lines(["-r", "5"])
    assert out == [buf.value.decode(), ""]
    # -w does not go with -N
    out, err = lines(["-N", "2", "-w", "t"], code=2)
    assert "usage" in err and out == [""]
