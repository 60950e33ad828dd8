"""The batched text scorer and sampler (rnn_amd_run_texts / _heads, rnn_amd_sample_texts) on wide and multi-head nets,
against the oracle, with the helpers and the bars of tests/test_gpu_run_texts.py and tests/test_gpu_sample_texts.py.  The
shapes of those two modules keep the forward plan (fwd_plan.h) on output=rows; the four nets here are the ones
tests/test_fwd_plan.py::test_the_batched_text_runs_shrinking_passes pins to the other forms, on the engine's scratch
rows (row0 = Scap + n_fwd = 16 for a net with its own BPTT, 17 for its forward clone):

  A  42 / 1024 / 42     trained for 600 generations: the hidden GEMM with nkt = 34 and ks = 7, 5, 7, 15 as the rows fall, k_fwd_finalize
                        over that many planes
  B  73 / 99 / 3650     tests/golden/multi-text-6c34c563i73-h99-o3650.net, 50 heads of 73: output=gemm with o_ks = 1, 2, 4 and
                        k_sum_slabs, 50 heads over the 4 waves of k_texts_step (13, 13, 12, 12), k_texts_continue on head 49
  C  128 / 512 / 4096   seeded weights, 32 heads of 128: output=wide (k_fwd_wide writing `out` at row0) from 128 rows on, below
                        that output=gemm with o_nkt = 17
  D  4 / 64 / 4         seeded weights: output=o4 (k_out_layer_o4) from 64 rows on, output=rows at 63

Every net starts from a seeded hidden row, half of it zeros as a rectifier leaves it (a zero row would hide a wrong hid0).
The fixture's metadata is the reference's older JSON form, which rnn_char_load_metadata does not read (neither does the
reference's: rnn_char_new_alphabet_from_net gives an empty alphabet), so B's alphabet is filled from the "alphabet" string
of that JSON and the text goes through rnn_char_alloc_encoded_text with it.

THE SCORER.  256 texts of lengths 2 (64 of them), 3 (64), 4 (64), 5 (1), 6 (62) and 7 (1), in a shuffled order, make the
passes of one call run at 256, 192, 128, 64, 63 and 1 rows (asserted: a(t) = the texts with len >= t + 2).  Two calls:
skips 0, where every row of every pass is part of a sum, and skips len - 2, where every sum is ONE step -- the one computed
at that text's last row count, so that a defect of one form shows undiluted in the sums of one length group (printed per
group).  Both at the project's parity bar, |got - want| <= 1e-4 |want|, against orc_cross_entropy /
orc_multi_cross_entropy.  Before the device is asked, on the oracle alone (printed, asserted): no scored probability
below 1e-29, the per-step log2 p spread over at least 3 bits, and on 8 texts zeroing rows 32 .. 64 of W_ho, or 32 rows of
W_ih, moves every sum -- in a heads call every head's -- by more than 100 bars.  The 8 texts are chosen on the oracle among
the 64 longest: without 32 rows a head's sum moves up or down, and of some hundred a few per cent stay within 1 % of where
they were whichever rows are taken, so not any 8 texts will do.  (The W_ih rows are I - 32 .. I for D; C's texts light only
the first 42 of its 128 input rows, B's sums hardly depend on its input rows, and not every text feeds A a symbol from 11
on: there the block was chosen on the oracle too, and is named where the net is made.)

THE SAMPLER.  test_gpu_sample_texts.checked with its limits: TOL 1e-4, at most max(1, 0.2 %) picks off the oracle's strict
pick, under 5 % of the steps close to a boundary; seeds chosen on the oracle so that its own run has no close step.  Two
heads from the same seeds must give different texts.

Largest relative differences measured on an MI355X (what by_group and at_the_bar print; the bar is 1e-4), one-step sums
per row count 256 / 192 / 128 / 64 / 63 / 1, then all steps:
  A                      1.2e-5  2.1e-5  1.1e-5  9.6e-8  1.3e-5  0        all steps 1.2e-5
  B, 50 heads            7.8e-6  7.8e-6  9.0e-6  5.5e-7  1.1e-5  9.8e-6   all steps 7.8e-6; worst head 33, head 49 8.0e-7
  B, 5 texts (5 .. 1)    3.4e-7  6.5e-6  4.7e-7  3.9e-7  5.9e-7           all steps 2.8e-6
  B, one softmax         1.0e-7  1.0e-7  4.4e-7  0       2.2e-6  3.9e-6   all steps 5.8e-7
  C, row0 16 and 17      6.5e-6  7.6e-6  8.6e-6  5.4e-6  9.1e-6  5.9e-6   all steps 6.5e-6 (the same figures at both)
  D                      8.0e-7  1.0e-5  1.8e-6  6.5e-8  3.0e-6  0        all steps 2.3e-6
  D, 64 texts (64 / 32 / 1) 8.0e-7  3.8e-6  3.7e-7; 63 texts (63 / 31 / 1) 1.5e-6  7.8e-7  0
(With scores twice as large C's sums reach down to 0.25 bits and differ by 9.6e-5 of their size; the oracle's own strict
and -Ofast builds differ by 7.4e-5 there.  At the size used those two differ by 8.7e-6.)
The sampler: in every batch no pick differs from the oracle's strict pick, no step is close to a boundary (the seeds were
chosen so), and every text is compared exactly."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import erewhon_case as ec
import recur_ctypes as rc
import sample_oracle as so
import scenarios as sc
from recur_amd.drivers import run_texts, sample_texts
from test_gpu_run_texts import BAR, at_the_bar, erewhon, forward_clone, oracle_like, oracle_sums
from test_gpu_sample_texts import checked

pytestmark = pytest.mark.gpu

LENS = [2] * 64 + [3] * 64 + [4] * 64 + [5] + [6] * 62 + [7]
ROWS = [256, 192, 128, 64, 63, 1]
GOLDEN_NET = os.path.join(rc.ROOT, "tests", "golden", "multi-text-6c34c563i73-h99-o3650.net")
KNOWS = (0.5, 42, 128, 0.125, 2.0)
_wide = {}
_wants = {}


@pytest.fixture(scope="module")
def amd():
    lib = rc.bind_char(rc.load_amd())
    assert lib.rnn_amd_device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return lib


class Wide:
    """what oracle_like and checked read of an AmdBatchedSet, for a net that is not one"""

    def __init__(self, lib, net, text, ih_block=None):
        n = net.contents
        self.lib, self.net, self.text = lib, net, text
        self.input_size, self.hidden_size, self.output_size = n.input_size, n.hidden_size, n.output_size
        self.I, self.H, self.O = n.i_size, n.h_size, n.o_size
        self.ih_block = ih_block or (self.I - 32, self.I)

    def sync(self):
        self.lib.rnn_amd_sync_host(self.net, rc.RNN_AMD_EVERYTHING)


def start_from(lib, net, seed):
    """a seeded hidden row, half of it zeros"""
    lib.rnn_amd_sync_host(net, rc.RNN_AMD_STREAM)
    n = net.contents
    h = rc.view(n.hidden_layer, n.h_size)
    h[:] = 0.0
    h[0] = 1.0
    h[1:1 + n.hidden_size] = np.maximum(np.random.default_rng(seed).standard_normal(n.hidden_size), 0.0) * 0.5
    lib.rnn_amd_host_written(net, rc.RNN_AMD_STREAM)
    return net


def seeded_net(lib, inputs, hidden, outputs, seed, top, knows=None):
    """Rectifier net with normal weights written from the host: bias row 0.1, recurrent rows 1 / sqrt(hidden), input rows
    `feed` (hidden values of about 1), W_ho top / sqrt(hidden) (scores with a standard deviation of about `top`).
    knows = (feed, used, alen, c, d): without 32 rows of weights that are noise a sum moves up as often as down, and of a
    text's 32 head sums a fifth hardly at all; so this net knows one thing, as a trained one does: hidden values 32 .. 64
    are driven (+d) by the input symbols 0 .. 32 and raise (+c) the `used` first scores of every head of alen -- the
    symbols its texts have.  Without rows 32 .. 64 of W_ho the symbols of a text lose probability in every head."""
    feed = knows[0] if knows else 1.0
    net = lib.rnn_new(inputs, hidden, outputs, rc.FLAG_STANDARD, seed, None, 4, 1e-3, 0.9, 0.0, rc.RELU)
    n = net.contents
    g = np.random.default_rng(seed)
    ih, ho = rc.view(n.ih_weights, n.i_size, n.h_size), rc.view(n.ho_weights, n.h_size, n.o_size)
    ih[:] = 0.0
    ho[:] = 0.0
    ih[0, 1:1 + hidden] = 0.1 * g.standard_normal(hidden)
    ih[1:1 + hidden, 1:1 + hidden] = g.standard_normal((hidden, hidden)) / np.sqrt(hidden)
    ih[1 + hidden:1 + hidden + inputs, 1:1 + hidden] = g.standard_normal((inputs, hidden)) * feed
    ho[:1 + hidden, :outputs] = g.standard_normal((1 + hidden, outputs)) * (top / np.sqrt(hidden))
    if knows:
        _, used, alen, c, d = knows
        ih[1 + hidden:1 + hidden + 32, 32:64] += d
        ho[32:64, :outputs].reshape(32, outputs // alen, alen)[:, :, :used] += c
    lib.rnn_amd_host_written(net, rc.RNN_AMD_WEIGHTS)
    return net


def golden_text(lib, net):
    """erewhon.txt in the symbols of the fixture's alphabet (the module's docstring: from the JSON the net carries)"""
    points = [ord(c) for c in json.loads(net.contents.metadata.decode("utf-8"))["alphabet"]]
    assert len(points) == net.contents.input_size == 73
    a = lib.rnn_char_new_alphabet()
    lib.rnn_char_alphabet_set_flags(a, False, True, False)  # as the JSON says: case sensitive, utf8, spaces kept
    for i, p in enumerate(points):
        a.contents.points[i] = p
    a.contents.len = len(points)
    raw = open(rc.EREWHON, "rb").read()
    n = C.c_int(0)
    p = lib.rnn_char_alloc_encoded_text(a, raw, len(raw), C.byref(n), None, False)
    text = np.ctypeslib.as_array(p, shape=(n.value,)).copy()
    lib.rnn_char_free_alphabet(a)
    assert text.max() < 73 and len(np.unique(text[30000:40000])) > 40
    return text


def wide(lib, name):
    """the four nets, made once and shared; their weights and hidden rows are not changed after this"""
    if name not in _wide:
        if name == "A":
            # trained(hidden=1024) for 600 generations instead of 60, then the hidden rows of W_ho times 4: of 1024 hidden
            # values 32 move the sums of the net after 60 generations by 0.1 %, of this one by 5 %.  Not every one of the
            # 8 texts feeds a symbol from 11 on (rows I - 32 .. I): the W_ih block is the first K tile
            w = sc.AmdBatchedSet(lib, **dict(ec.KW, hidden_size=1024))
            w.load_text(np.ascontiguousarray(erewhon()[:20000]))
            for i in range(600):
                lib.rnn_amd_set_char_step(w.handle, i, rc.WEIGHTED, 0.9)
            w.sync()
            rc.view(w.net.contents.ho_weights, w.H, w.O)[1:] *= np.float32(4.0)
            lib.rnn_amd_host_written(w.net, rc.RNN_AMD_WEIGHTS)
            w.text, w.ih_block = erewhon(), (0, 32)
        elif name == "B":
            net = lib.rnn_load_net(GOLDEN_NET.encode())
            # (the sums hardly depend on this net's input rows: without rows 144 .. 176 they move by 0.6 % in the median;
            # its first K tile, the bias and 31 hidden values, moves every one of them by more than 3 %)
            w = Wide(lib, net, golden_text(lib, net), ih_block=(0, 32))
        elif name == "C":
            # rows 513 .. 555 of W_ih are the 42 symbols the text has, the first 32 of them the block
            w = Wide(lib, seeded_net(lib, 128, 512, 4096, 21, 1.0, knows=KNOWS), erewhon(128), ih_block=(513, 545))
        else:
            w = Wide(lib, seeded_net(lib, 4, 64, 4, 22, 2.0), erewhon(4))
        start_from(lib, w.net, 5)
        _wide[name] = w
    return _wide[name]


def a_clone(lib, w):
    return start_from(lib, forward_clone(lib, w.net), 6)


def design(w, lens=LENS, at=30000, seed=3):
    """texts of these lengths from the net's text, in a shuffled order; the row count of every pass"""
    lens = [int(x) for x in np.random.default_rng(seed).permutation(lens)]
    texts = [np.ascontiguousarray(w.text[at + 37 * k:at + 37 * k + n]) for k, n in enumerate(lens)]
    rows = [sum(n >= t + 2 for n in lens) for t in range(max(lens) - 1)]
    return texts, lens, rows


def head_sums(o, texts, skips, alen):
    """oracle_sums for an output row of heads of alen (orc_multi_cross_entropy, charmodel-multi-predict.c:383-408)"""
    heads = o.output_size // alen
    want = np.zeros((len(texts), heads))
    for k, (t, skip) in enumerate(zip(texts, skips)):
        if len(t) - 1 > skip:
            ent = (C.c_double * heads)(*([0.0] * heads))
            o.orc.orc_multi_cross_entropy(o.z, k, rc.u8ptr(t), len(t), alen, ent, skip)
            want[k] = -np.array(ent[:]) * (len(t) - skip - 1)
    return want


def sums_of(o, start, texts, skips, alen):
    o.arrays()["hidden"][:] = start
    return head_sums(o, texts, skips, alen) if alen else oracle_sums(o, texts, skips)


def step_probabilities(o, start, texts, alen):
    """the oracle alone, step by step as orc_cross_entropy goes: the probability of every scored symbol, [steps][heads]"""
    o.arrays()["hidden"][:] = start
    alen = alen or o.output_size
    heads = o.output_size // alen
    p, out = np.zeros(alen, np.float32), []
    for k, t in enumerate(texts):
        for i in range(len(t) - 1):
            ans = np.ctypeslib.as_array(o.orc.orc_one_hot_opinion(o.z, k, int(t[i]), 0.0), shape=(o.O,))
            row = []
            for h in range(heads):
                o.orc.orc_softmax(rc.fptr(p), rc.fptr(ans[h * alen:(h + 1) * alen]), alen)
                row.append(float(p[int(t[i + 1])]))
            out.append(row)
    return np.array(out)


def conditions(lib, w, net, texts, alen, what, ho_block=(32, 64)):
    """Checked on the oracle alone: the scored probabilities, their spread, and that 32 rows of either weight matrix show
    in every sum of 8 of the longest texts.  Returns the wants of the two calls."""
    o = oracle_like(lib, w, net, len(texts))
    start = o.arrays()["hidden"].copy()
    p = step_probabilities(o, start, texts, alen)
    bits = np.log2(p)
    print("%s: %d steps x %d heads, lowest scored probability %.3g, log2 p from %.2f to %.2f (%.1f bits)"
          % (what, p.shape[0], p.shape[1], p.min(), bits.min(), bits.max(), bits.max() - bits.min()))
    assert p.min() > 1e-29 and bits.max() - bits.min() >= 3.0
    lens = [len(t) for t in texts]
    want0 = sums_of(o, start, texts, [0] * len(texts), alen)
    want1 = sums_of(o, start, texts, [n - 2 for n in lens], alen)
    # the two wants are those steps: all of them, and the last of each text
    ends = np.cumsum([n - 1 for n in lens])
    assert np.allclose(want1.reshape(len(texts), -1), bits[ends - 1], rtol=1e-6, atol=0)
    assert np.allclose(want0.reshape(len(texts), -1), np.add.reduceat(bits, ends - [n - 1 for n in lens]), rtol=1e-6, atol=0)
    if len(texts) >= 8:
        # the texts are chosen on the oracle: of the (up to 64) longest, the first 8 whose EVERY sum -- every head's --
        # moves by more than 100 bars without either block
        cand = np.argsort([-n for n in lens], kind="stable")[:64]
        some = [texts[k] for k in cand]
        base = want0[cand].reshape(len(cand), -1)
        moves = {}
        for name, (lo, hi) in (("ho_w", ho_block), ("ih_w", w.ih_block)):
            m = o.arrays()[name]
            kept = m[lo:hi].copy()
            m[lo:hi] = 0.0
            moved = sums_of(o, start, some, [0] * len(some), alen).reshape(len(cand), -1) - base
            m[lo:hi] = kept
            moves[name] = np.abs(moved) / np.abs(base)
        every = np.minimum(moves["ho_w"], moves["ih_w"]).min(axis=1) > 100 * BAR
        chosen = np.nonzero(every)[0][:8]
        print("%s: of the %d longest texts %d have every sum moved by both blocks; the first 8: texts %s of lengths %s"
              % (what, len(cand), every.sum(), [int(k) for k in cand[chosen]], [lens[k] for k in cand[chosen]]))
        assert len(chosen) == 8
        for name, (lo, hi) in (("ho_w", ho_block), ("ih_w", w.ih_block)):
            least = moves[name][chosen].min()
            print("%s: without rows %d .. %d of %s every one of the %d sums of these 8 texts moves by at least %.3g of its "
                  "size (%.0f bars)" % (what, lo, hi, name, moves[name][chosen].size, least, least / BAR))
            assert least > 100 * BAR
    o.close()
    return want0, want1


def by_group(got, want, lens, rows, what):
    """the largest relative difference of the one-step sums per length group: the form run at that row count"""
    got, want = np.asarray(got).reshape(len(lens), -1), np.asarray(want).reshape(len(lens), -1)
    rel = np.abs(got - want) / np.abs(want)
    for t, r in enumerate(rows):
        mine = np.array(lens) == t + 2
        if mine.any():
            print("%s: scored at %3d rows (%3d texts of length %d): largest relative difference %.3g"
                  % (what, r, mine.sum(), t + 2, rel[mine].max()))
    if got.shape[1] > 1:
        worst = rel.max(axis=0)
        print("%s: per head, largest %.3g (head %d), head 0 %.3g, last head %.3g"
              % (what, worst.max(), worst.argmax(), worst[0], worst[-1]))


def scored(lib, w, net, key, alen=0, lens=LENS, rows=None, what="", keep=None, ho_block=(32, 64)):
    """the two calls of the module's docstring on one batch"""
    texts, lens, passes = design(w, lens)
    if keep is not None:
        texts = [texts[k] for k in keep]
        lens = [lens[k] for k in keep]
        passes = [sum(n >= t + 2 for n in lens) for t in range(max(lens) - 1)]
    print("%s: passes at %s rows" % (what, passes))
    if rows is not None:
        assert passes == rows
    if key not in _wants:
        _wants[key] = conditions(lib, w, net, texts, alen, what, ho_block)
    want0, want1 = _wants[key]
    got0 = run_texts(lib, net, texts, [0] * len(texts), alphabet_len=alen)
    got1 = run_texts(lib, net, texts, [n - 2 for n in lens], alphabet_len=alen)
    by_group(got1, want1, lens, passes, what)
    at_the_bar(got0, want0, what + ", every step:")
    at_the_bar(got1, want1, what + ", the last step:")


def test_scores_hidden_1024(amd):
    w = wide(amd, "A")
    net = a_clone(amd, w)
    scored(amd, w, net, "A", rows=ROWS, what="A 42/1024/42")
    amd.rnn_delete_net(net)


def test_scores_50_heads_of_73(amd):
    w = wide(amd, "B")
    net = a_clone(amd, w)
    scored(amd, w, net, "B", alen=73, rows=ROWS, what="B 73/99/3650, 50 heads")
    scored(amd, w, net, "B5", alen=73, lens=[2, 3, 4, 5, 6], rows=[5, 4, 3, 2, 1], what="B, 5 texts")
    amd.rnn_delete_net(net)


def test_scores_one_softmax_over_3650(amd):
    """the plain call on B's whole row, on the texts whose every symbol the oracle gives more than 1e-29"""
    w = wide(amd, "B")
    net = a_clone(amd, w)
    texts, lens, _ = design(w)
    o = oracle_like(amd, w, net, len(texts))
    p = step_probabilities(o, o.arrays()["hidden"].copy(), texts, 0)[:, 0]
    o.close()
    ends = np.cumsum([n - 1 for n in lens])
    keep = [k for k, n in enumerate(lens) if p[ends[k] - (n - 1):ends[k]].min() > 1e-29]
    print("%d of %d texts kept" % (len(keep), len(texts)))
    assert len(keep) >= 128 and {lens[k] for k in keep} == set(LENS)
    # the first pass at 193 rows or more is planned o_ks = 1, the passes at 64 rows or fewer o_ks = 4 (test_fwd_plan.py)
    lens = [lens[k] for k in keep]
    passes = [sum(n >= t + 2 for n in lens) for t in range(max(lens) - 1)]
    assert passes[0] >= 193 and sum(r <= 64 for r in passes) >= 2 and passes[-1] >= 1
    # (over the whole row rows 32 .. 64 of W_ho move some of these sums by 49 bars only; rows 0 .. 32 were chosen)
    scored(amd, w, net, "B whole", keep=keep, rows=passes, what="B, one softmax over 3650", ho_block=(0, 32))
    amd.rnn_delete_net(net)


def test_scores_32_heads_of_128_at_an_even_and_an_odd_row0(amd):
    """row0 = Scap + n_fwd (texts_api.c): Scap is 16 for this engine's one training net, and n_fwd counts the engine's
    live forward clones -- none while the net itself is scored (every test here deletes its clone, and a deleted clone
    leaves the count), one while its clone is.  So the order of the two calls matters: 16, then 17."""
    w = wide(amd, "C")
    start_from(amd, w.net, 6)  # the clone's start, so that one reference serves both
    try:
        scored(amd, w, w.net, "C", alen=128, rows=ROWS, what="C 128/512/4096, 32 heads, the net itself")
        net = a_clone(amd, w)
        scored(amd, w, net, "C", alen=128, rows=ROWS, what="C 128/512/4096, 32 heads, a forward clone")
        amd.rnn_delete_net(net)
    finally:
        start_from(amd, w.net, 5)


def test_scores_4_outputs_at_64_and_63_rows(amd):
    w = wide(amd, "D")
    net = a_clone(amd, w)
    scored(amd, w, net, "D", rows=ROWS, what="D 4/64/4")
    scored(amd, w, net, "D64", lens=[2] * 32 + [3] * 31 + [4], rows=[64, 32, 1], what="D, 64 texts")
    scored(amd, w, net, "D63", lens=[2] * 32 + [3] * 30 + [4], rows=[63, 31, 1], what="D, 63 texts")
    amd.rnn_delete_net(net)


def clean_seeds(lib, w, net, first, max_len, bias, alen=None, head=0):
    """on the oracle alone, as test_gpu_sample_texts.clean_seeds: for every text the next seed whose run from first[k] has
    no step within TOL of a boundary"""
    o = oracle_like(lib, w, net, 1)
    start = o.arrays()["hidden"].copy()
    seeds, seed = [], 0
    for f in first:
        while True:
            seed += 1
            o.arrays()["hidden"][:] = start
            if not so.free_run(o, 0, f, seed, max_len, bias, alen=alen, head=head)[1]:
                break
        seeds.append(seed)
    o.close()
    print("%d seeds out of the first %d" % (len(seeds), seed))
    assert seed < 2 * len(first)
    return seeds


def sampled(lib, w, net, n, max_len, bias, alen=0, head=0, what=""):
    symbols = alen or w.output_size
    first = [(5 * k + 1) % min(symbols, w.input_size) for k in range(n)]
    greedy = bias >= so.GREEDY_BIAS
    seeds = list(range(1, n + 1)) if greedy else clean_seeds(lib, w, net, first, max_len, bias, alen or None, head)
    texts, _ = checked(lib, w, net, first, seeds, max_len, bias, alphabet_len=alen, head=head,
                       what="%s, %d texts, bias %g" % (what, n, bias))
    assert greedy or len({t.tobytes() for t in texts}) > n // 4
    return first, seeds, texts


def other_head(lib, net, first, seeds, texts, max_len, bias, alen, head):
    other, _ = sample_texts(lib, net, first, seeds, max_len, bias, alphabet_len=alen, head=head)
    differ = sum(not np.array_equal(x, y) for x, y in zip(other, texts))
    print("head %d against the texts above: %d of %d differ" % (head, differ, len(texts)))
    assert differ > len(texts) // 2


@pytest.mark.parametrize("n", [256, 17])
def test_samples_hidden_1024(amd, n):
    w = wide(amd, "A")
    net = a_clone(amd, w)
    for bias in (0.0, 1.0):
        sampled(amd, w, net, n, 4 if n == 256 else 6, bias, what="A 42/1024/42")
    amd.rnn_delete_net(net)


@pytest.mark.parametrize("n", [256, 64])
def test_samples_heads_of_73(amd, n):
    w = wide(amd, "B")
    net = a_clone(amd, w)
    max_len = 4 if n == 256 else 6
    for head in (0, 17, 49):
        first, seeds, texts = sampled(amd, w, net, n, max_len, 0.0, alen=73, head=head, what="B head %d of 50" % head)
        other_head(amd, net, first, seeds, texts, max_len, 0.0, 73, (head + 1) % 50)
    if n == 64:
        sampled(amd, w, net, n, max_len, 200.0, alen=73, head=49, what="B head 49 of 50, greedy")
    amd.rnn_delete_net(net)


@pytest.mark.parametrize("head", [0, 31])
@pytest.mark.parametrize("n", [256, 64])
def test_samples_heads_of_128(amd, n, head):
    """256 rows: output=wide; 64: output=gemm"""
    w = wide(amd, "C")
    net = a_clone(amd, w)
    max_len = 4 if n == 256 else 6
    first, seeds, texts = sampled(amd, w, net, n, max_len, 0.0, alen=128, head=head, what="C head %d of 32" % head)
    other_head(amd, net, first, seeds, texts, max_len, 0.0, 128, 31 - head)
    amd.rnn_delete_net(net)


def test_a_first_symbol_above_255(amd):
    """first[k] is an int in [0, input_size), not a byte: on a net of 300 inputs the symbols 256 .. 299 are fed as they
    are.  Six texts from 0, 255, 256, 257, 298 and 299 against the oracle, drawn and greedy; then two rows from 0 and 256
    with ONE seed, chosen on the oracle so that its two texts differ and neither has a close step: a first symbol cut to
    its low byte would make the device's two texts equal."""
    lib = amd
    w = Wide(lib, start_from(lib, seeded_net(lib, 300, 40, 48, 23, 2.0), 5), None)
    net = a_clone(lib, w)
    first = [0, 255, 256, 257, 298, 299]
    checked(lib, w, net, first, clean_seeds(lib, w, net, first, 8, 0.0), 8, 0.0, what="300 inputs, bias 0")
    checked(lib, w, net, first, list(range(1, 7)), 8, 200.0, what="300 inputs, greedy")
    o = oracle_like(lib, w, net, 1)
    start = o.arrays()["hidden"].copy()
    for seed in range(1, 100):
        runs = []
        for f in (0, 256):
            o.arrays()["hidden"][:] = start
            runs.append(so.free_run(o, 0, f, seed, 8, 0.0))
        if not runs[0][1] and not runs[1][1] and not np.array_equal(runs[0][0], runs[1][0]):
            break
    else:
        raise AssertionError("no seed below 100 tells symbol 0 from symbol 256 on the oracle")
    o.close()
    print("seed %d: the oracle from 0 %s, from 256 %s" % (seed, list(runs[0][0]), list(runs[1][0])))
    pair, _ = checked(lib, w, net, [0, 256], [seed, seed], 8, 0.0, what="0 and 256, one seed")
    assert not np.array_equal(pair[0], pair[1])
    lib.rnn_delete_net(net)
    lib.rnn_delete_net(w.net)


@pytest.mark.parametrize("n", [64, 63])
def test_samples_4_outputs(amd, n):
    """64 rows: output=o4; 63: output=rows"""
    w = wide(amd, "D")
    net = a_clone(amd, w)
    for bias in (0.0, 1.0):
        sampled(amd, w, net, n, 6, bias, what="D 4/64/4")
    amd.rnn_delete_net(net)
