"""Many texts against one net in one batched device run (rnn_amd_run_texts, rnn_amd_run_texts_heads,
rnn_amd_char_cross_entropy_texts; recur_amd/csrc/texts_api.c, texts_plan.h, k_texts_step in kernels_rows.hip) against the
oracle: an OracleSet with one stream per text, the product net's weights copied in, every stream's hidden row set to the
product net's hidden row, then orc_cross_entropy (charmodel-predict.c:62-80) per stream, times -(len - skip - 1) to undo
its division.  The bar is the project's parity bar, |got - want| <= 1e-4 |want|; where nothing is scored the sum is
exactly 0.0 (the oracle is not asked then: its skip loop would read past the text, charmodel-predict.c:67-69).

The nets are erewhon_case.KW-shaped, trained for 60 generations so that entropies are a few bits -- far from 0 and from the
-100 cap of capped_log2f.  Texts are slices of the erewhon text.

With 42, 73 or 3 x 14 outputs and 39 to 256 hidden values every forward pass of this module is planned output=rows
(k_out_layer; fwd_plan.h).  The other output-layer forms on these rows -- the MFMA GEMM with k_sum_slabs, k_fwd_wide,
k_out_layer_o4 --, more heads than k_texts_step has waves, and hidden 1024 are tests/test_gpu_texts_wide.py's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import erewhon_case as ec
import recur_ctypes as rc
import scenarios as sc
from recur_amd.drivers import run_texts, text_pointers

pytestmark = pytest.mark.gpu
BAR = 1e-4
_nets = {}


@pytest.fixture(scope="module")
def amd():
    lib = rc.bind_char(rc.load_amd())
    assert lib.rnn_amd_device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return lib


def erewhon(symbols=None):
    text = ec.encoded_text()
    return text if symbols is None else np.ascontiguousarray(text % symbols)


def trained(lib, hidden=99, symbols=42, outputs=None, text_symbols=None):
    """A training set of 4 streams after 60 generations on the erewhon text (momentum 0.9), shared by the tests of this
    module; its weights are not changed after that (a test that wants other weights writes them back)."""
    key = (hidden, symbols, outputs, text_symbols)
    if key not in _nets:
        kw = dict(ec.KW, hidden_size=hidden, input_size=symbols, output_size=outputs or symbols)
        a = sc.AmdBatchedSet(lib, **kw)
        a.load_text(np.ascontiguousarray(erewhon(text_symbols)[:20000]))
        for i in range(60):
            lib.rnn_amd_set_char_step(a.handle, i, rc.WEIGHTED, 0.9)
        _nets[key] = a
    return _nets[key]


def forward_clone(lib, net):
    # text-predict.c:538-541: borrows the weights, no bptt
    return lib.rnn_clone(net, net.contents.flags & ~(rc.FLAG_OWN_BPTT | rc.FLAG_OWN_WEIGHTS), rc.SUBSEED, None)


def hidden_row(lib, net):
    lib.rnn_amd_sync_host(net, rc.RNN_AMD_STREAM)
    return rc.view(net.contents.hidden_layer, net.contents.h_size).copy()


def rng_of(lib, net):
    lib.rnn_amd_sync_host(net, rc.RNN_AMD_STREAM)
    r = net.contents.rng
    return (r.a, r.b, r.c, r.d)


def oracle_like(lib, a, net, S):
    """S oracle streams with a's weights, every one starting from net's hidden row"""
    a.sync()
    n = a.net.contents
    o = sc.OracleSet(input_size=a.input_size, hidden_size=a.hidden_size, output_size=a.output_size, S=S, D=1,
                     activation=n.activation, learn_rate=1e-3, seed=1)
    o.arrays()["ih_w"][:] = rc.view(n.ih_weights, a.I, a.H)
    o.arrays()["ho_w"][:] = rc.view(n.ho_weights, a.H, a.O)
    o.arrays()["hidden"][:] = hidden_row(lib, net)[None, :]
    return o


def oracle_sums(o, texts, skips):
    want = np.zeros(len(texts))
    for k, (t, skip) in enumerate(zip(texts, skips)):
        if len(t) - 1 > skip:  # something is scored
            want[k] = o.orc.orc_cross_entropy(o.z, k, rc.u8ptr(t), len(t), skip) * -(len(t) - skip - 1)
    return want


def at_the_bar(got, want, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    rel = np.abs(got - want) / np.where(want != 0, np.abs(want), 1.0)
    print("%s largest relative difference %.3g over %d sums (|want| %.3g .. %.3g)"
          % (what, rel[want != 0].max() if (want != 0).any() else 0.0, want.size, np.abs(want).min(), np.abs(want).max()))
    assert np.all(got[want == 0] == 0.0), (got[want == 0])
    assert np.all(np.abs(got - want) <= BAR * np.abs(want)), (got, want)


def slices(starts_lens, symbols=None):
    text = erewhon(symbols)
    return [np.ascontiguousarray(text[a:a + n]) for a, n in starts_lens]


def test_a_ragged_batch(amd):
    """equal lengths, a skip at or past len - 1 (nothing scored), empty and one-symbol texts"""
    a = trained(amd)
    net = forward_clone(amd, a.net)
    lens = [600, 1, 2, 3, 64, 65, 600, 0]
    skips = [5, 0, 0, 5, 0, 10, 0, 0]
    texts = slices(zip([30000, 31000, 32000, 33000, 34000, 35000, 36000, 37000], lens))
    assert not np.array_equal(texts[0], texts[6])
    o = oracle_like(amd, a, net, len(texts))
    got = run_texts(amd, net, texts, skips)
    want = oracle_sums(o, texts, skips)
    assert list(want != 0) == [True, False, True, False, True, True, True, False]
    at_the_bar(got, want, "ragged")
    # no skips is all zeros
    at_the_bar(run_texts(amd, net, texts[2:6]), oracle_sums(oracle_like(amd, a, net, 4), texts[2:6], [0] * 4), "skips NULL")
    o.close()
    amd.rnn_delete_net(net)


@pytest.mark.parametrize("kind", ["training", "forward"])
def test_the_start_state_is_taken_and_left_alone(amd, kind):
    lib = amd
    a = trained(lib)
    if kind == "training":
        net, twin = a.nets[0], a.nets[1]  # both with bptt: the same per-net path
    else:
        net, twin = forward_clone(lib, a.net), forward_clone(lib, a.net)
    # the twin starts where the net starts
    lib.rnn_amd_sync_host(twin, rc.RNN_AMD_STREAM)
    rc.view(twin.contents.hidden_layer, a.H)[:] = hidden_row(lib, net)
    lib.rnn_amd_host_written(twin, rc.RNN_AMD_STREAM)
    texts = slices([(30000, 50), (31000, 120), (32000, 33)])
    skips = [0, 5, 2]
    unprimed = run_texts(lib, net, texts, skips)
    prefix = np.ascontiguousarray(erewhon()[29000:29100])
    for x in (net, twin):
        assert lib.rnn_char_prime(x, None, rc.u8ptr(prefix), len(prefix)) == int(prefix[-1])
    hid, rng = hidden_row(lib, net), rng_of(lib, net)
    assert np.array_equal(hid, hidden_row(lib, twin))
    o = oracle_like(lib, a, net, len(texts))
    got = run_texts(lib, net, texts, skips)
    at_the_bar(got, oracle_sums(o, texts, skips), "primed " + kind)
    print("primed - unprimed", got - unprimed)
    assert np.all(np.abs(got - unprimed) > 1e-6)
    # the net is where it was: hidden row bit for bit, generator, and what it computes next
    assert np.array_equal(hidden_row(lib, net), hid) and rng_of(lib, net) == rng
    seg = texts[1]
    mine = lib.rnn_char_cross_entropy(net, None, rc.u8ptr(seg), len(seg), 3, None, 0)
    twins = lib.rnn_char_cross_entropy(twin, None, rc.u8ptr(seg), len(seg), 3, None, 0)
    print("after the batch", mine, "a twin that never saw it", twins)
    assert mine == twins
    o.close()
    if kind == "forward":
        lib.rnn_delete_net(twin)
        lib.rnn_delete_net(net)


def test_two_waves_and_every_small_row_count(amd):
    """300 texts of 0 .. 40 symbols: two waves at the default width, and within a wave the forward launchers run at
    every row count from many down to 1"""
    a = trained(amd, hidden=39)
    net = forward_clone(amd, a.net)
    rng = np.random.default_rng(11)
    lens = [k % 41 for k in range(300)]
    skips = [int(x) for x in rng.integers(0, 8, 300)]
    texts = slices((30000 + 37 * k, n) for k, n in enumerate(lens))
    o = oracle_like(amd, a, net, 300)
    got = run_texts(amd, net, texts, skips)
    want = oracle_sums(o, texts, skips)
    at_the_bar(got, want, "300 texts")
    # a second, narrower call finds its rows where the first left them (other rows and row counts: the bar, not the bits)
    at_the_bar(run_texts(amd, net, texts[100:200], skips[100:200]), want[100:200], "100 of them again")
    o.close()
    amd.rnn_delete_net(net)


@pytest.mark.parametrize("hidden,symbols", [(39, 42), (99, 42), (130, 73), (256, 42)])
def test_shapes(amd, hidden, symbols):
    a = trained(amd, hidden=hidden, symbols=symbols)
    net = forward_clone(amd, a.net)
    texts = slices([(30000, 200), (31000, 2), (32000, 77), (33000, 130), (34000, 9)])
    skips = [5, 0, 0, 3, 1]
    o = oracle_like(amd, a, net, len(texts))
    at_the_bar(run_texts(amd, net, texts, skips), oracle_sums(o, texts, skips), "hidden %d, %d symbols" % (hidden, symbols))
    o.close()
    amd.rnn_delete_net(net)


def test_heads(amd):
    """an output row of 3 heads of 14 symbols against orc_multi_cross_entropy (charmodel-multi-predict.c:383-408)"""
    lib = amd
    a = trained(lib, hidden=99, symbols=42, text_symbols=14)
    net = forward_clone(lib, a.net)
    lens, skips = [40, 2, 17, 1, 33, 40], [0, 0, 3, 0, 40, 5]
    texts = slices(zip([30000, 31000, 32000, 33000, 34000, 35000], lens), symbols=14)
    o = oracle_like(lib, a, net, len(texts))
    want = np.zeros((len(texts), 3))
    for k, (t, skip) in enumerate(zip(texts, skips)):
        if len(t) - 1 > skip:
            ent = (C.c_double * 3)(0.0, 0.0, 0.0)
            o.orc.orc_multi_cross_entropy(o.z, k, rc.u8ptr(t), len(t), 14, ent, skip)
            want[k] = -np.array(ent[:]) * (len(t) - skip - 1)
    got = run_texts(lib, net, texts, skips, alphabet_len=14)
    assert got.shape == (6, 3) and (want[0] != 0).all() and not want[3].any() and not want[4].any()
    at_the_bar(got, want, "3 heads of 14")
    # one head as wide as the row is the plain call
    whole = run_texts(lib, net, texts, skips, alphabet_len=42)
    assert whole.shape == (6, 1) and np.array_equal(whole[:, 0], run_texts(lib, net, texts, skips))
    o.close()
    lib.rnn_delete_net(net)


def test_the_soft_clip_in_the_feed_half(amd):
    """With the recurrent weights doubled the hidden values grow from symbol to symbol until an input row sums to more
    than 16 per element and maybe_scale_inputs (recur-nn.c:68-81) scales it -- by about 0.9 here, which moves the
    figures far more than the bar.  The exploded net's softmax is nearly one-hot, so only the steps whose next symbol it
    still gives a representable probability are scored (the skips): found by stepping the oracle over the erewhon text,
    and checked on the oracle below before the device is asked.  (Between the oracle's strict and -Ofast builds these
    sums differ by up to 8e-6 of their size.)"""
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
        starts, lens, skips = [30290, 32088, 32581, 33741, 33683], [12, 12, 12, 12, 12], [9, 10, 10, 10, 9]
        texts = slices(zip(starts, lens))
        assert max(lens) <= 30
        nt = len(texts)
        o = oracle_like(lib, a, net, 2 * nt)
        # on the oracle alone: the clip fires in every text, at or before its last step, and no scored probability is
        # within a factor of 10 of capped_log2f's 1e-30
        probs = np.zeros(a.O, np.float32)
        for k, (t, skip) in enumerate(zip(texts, skips)):
            fired, low = [], 1.0
            for i in range(len(t) - 1):
                # the row rnn_opinion is about to build: bias, hidden values, one symbol (recur-nn.c:104-112)
                row_sum = 1.0 + float(o.arrays()["hidden"][nt + k][1:a.hidden_size + 1].astype(np.float64).sum()) + 1.0
                fired.append(row_sum > a.I * 16)
                ans = o.orc.orc_one_hot_opinion(o.z, nt + k, int(t[i]), 0.0)
                if i >= skip:
                    o.orc.orc_softmax(rc.fptr(probs), ans, a.output_size)
                    low = min(low, float(probs[int(t[i + 1])]))
            print("text %d: clipped steps %s, lowest scored probability %.3g" % (k, np.nonzero(fired)[0], low))
            assert any(fired) and low > 1e-29
        want = oracle_sums(o, texts, skips)
        got = run_texts(lib, net, texts, skips)
        at_the_bar(got, want, "soft clip")
        o.close()
        lib.rnn_delete_net(net)
    finally:
        lib.rnn_amd_sync_host(a.net, rc.RNN_AMD_WEIGHTS)
        ih[:] = kept
        lib.rnn_amd_host_written(a.net, rc.RNN_AMD_WEIGHTS)


def same_figure(got, want):
    if np.isnan(want) or np.isinf(want):
        return (np.isnan(got) and np.isnan(want)) or got == want
    return got == 0.0 if want == 0.0 else abs(got - want) <= BAR * abs(want)


@pytest.mark.parametrize("with_prefix", [False, True])
def test_the_char_layer_is_the_per_text_call_on_fresh_clones(amd, with_prefix):
    lib = amd
    a = trained(lib)
    texts = slices([(30000, 50), (31000, 1), (32000, 0), (33000, 2), (34000, 120), (35000, 7)])
    prefix = np.ascontiguousarray(erewhon()[29000:29040]) if with_prefix else None
    pp, pl = (rc.u8ptr(prefix), len(prefix)) if with_prefix else (None, 0)
    keep, ptrs, lens = text_pointers(texts)
    for ignore_first in (0, 5):
        net = forward_clone(lib, a.net)
        got = np.full(len(texts), 123.0)
        assert lib.rnn_amd_char_cross_entropy_texts(net, None, ptrs, rc.iptr(lens), len(texts), ignore_first, pp, pl,
                                                    got.ctypes.data_as(C.POINTER(C.c_double))) == 0
        lib.rnn_delete_net(net)
        want = []
        for t in keep:
            c = forward_clone(lib, a.net)
            want.append(lib.rnn_char_cross_entropy(c, None, rc.u8ptr(t) if len(t) else None, len(t), ignore_first, pp, pl))
            lib.rnn_delete_net(c)
        print("ignore_first", ignore_first, "batch", got, "per text", want)
        assert all(same_figure(g, w) for g, w in zip(got, want))
        assert 1.0 < got[0] < 6.0 and 1.0 < got[4] < 6.0  # a few bits per symbol


def test_the_tool_scores_files_independently_with_I_and_as_before_without(amd, tmp_path):
    lib = amd
    build = os.path.join(rc.ROOT, "build")
    path = str(tmp_path / "erewhon.net")
    r = subprocess.run([os.path.join(build, "text_predict_amd"), "-f", rc.EREWHON, "-H", "99", "-t", "16", "-d", "10",
                        "-l", "1e-3", "-s", "60", "-r", "60", "-V", "1500", "-n", path],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0 and os.path.exists(path), r.stderr[-2000:]
    raw = open(rc.EREWHON, "rb").read()
    files = []
    for k, (at, n) in enumerate([(20000, 400), (26000, 300), (31000, 150)]):
        files.append(tmp_path / ("part%d.txt" % k))
        files[-1].write_bytes(raw[at:at + n])
    names = [str(f) for f in files]
    tool = [os.path.join(build, "text_cross_entropy_amd"), "-f", path, "-i", "5", "-p", "the "]

    def figures(args):
        r = subprocess.run(args, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-2000:]
        rows = [line.rsplit(" ", 1) for line in r.stdout.strip().splitlines()]
        assert [x[0] for x in rows] == names  # one line per file, in argument order
        return np.array([float(x[1]) for x in rows])

    def encode(alphabet, data):
        n = C.c_int(0)
        p = lib.rnn_char_alloc_encoded_text(alphabet, data, len(data), C.byref(n), None, False)
        return np.ctypeslib.as_array(p, shape=(n.value,)).copy()

    net = lib.rnn_load_net(path.encode())
    alphabet = lib.rnn_char_new_alphabet_from_net(net)
    texts = [encode(alphabet, f.read_bytes()) for f in files]
    prefix = encode(alphabet, b"the ")
    # without -I: one net, the state carried from file to file (and the prefix in front of each), as it always was
    carried = [lib.rnn_char_cross_entropy(net, alphabet, rc.u8ptr(t), len(t), 5, rc.u8ptr(prefix), len(prefix)) for t in texts]
    lib.rnn_delete_net(net)
    plain = figures(tool + names)
    print("plain", plain, "library", carried)
    assert np.all(np.abs(plain - carried) < 1e-5)
    # with -I: the prefix once, then every file on its own
    net = lib.rnn_load_net(path.encode())
    keep, ptrs, lens = text_pointers(texts)
    want = np.zeros(3)
    assert lib.rnn_amd_char_cross_entropy_texts(net, alphabet, ptrs, rc.iptr(lens), 3, 5, rc.u8ptr(prefix), len(prefix),
                                                want.ctypes.data_as(C.POINTER(C.c_double))) == 0
    independent = figures(tool + ["-I"] + names)
    print("-I", independent, "library", want)
    assert np.all(np.abs(independent - want) < 1e-5)
    assert np.all(independent[1:] != plain[1:])  # the carried state shows from the second file on
    lib.rnn_char_free_alphabet(alphabet)
    lib.rnn_delete_net(net)
