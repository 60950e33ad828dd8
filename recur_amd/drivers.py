"""Small drivers of librecur_amd.so's C API that benchmarks, tools and tests share.

``ApiSet`` drives a library that speaks the recur-nn.h ABI (librecur_amd.so through its per-net drop-in calls; the
tests also point it at the compiled reference) exactly the way the reference's own caller does (rnn_char_epoch,
charmodel-predict.c:288-311).  ``AmdBatchedSet`` drives the additive batched entry points (include/recur_amd.h
part 2): the whole set per call, text on the device.  ``run_texts`` scores a list of encoded texts against one net in
one batched call (rnn_amd_run_texts / _heads), ``sample_texts`` draws a batch of texts from one net in one batched call
(rnn_amd_sample_texts), ``continue_texts`` continues a batch of prompts (rnn_amd_continue_texts), ``trace_texts`` hands
back the scorer's figures symbol by symbol (rnn_amd_trace_texts); ``run_texts_from``, ``trace_texts_from`` and
``continue_texts_from`` are those with a start state per text and the final states handed back, as numpy arrays
[n][h_size] (the rnn_amd_*_texts_from calls); ``run_sequences`` runs a list of dense feature sequences against one net in
one batched call (rnn_amd_run_sequences): per frame the class groups' probabilities and winners, with states in and out
in the same form; ``classify_texts`` runs a list of encoded texts against one classifier net in one batched call
(rnn_amd_classify_texts): per text the sums and sums of squares of every class's probability and the score against the
symbols' classes; ``run_automaton`` plays rnnca's automaton from a seed frame on an ``AutomatonGeometry`` in one call
(rnn_amd_run_automaton): the frames as uint8 [n][3][height][width] and the cells' states, and ``parse_offsets`` expands an
offset pattern (rnn_amd_automaton_parse_offsets); ``dream_sequences`` runs parrot's player, many closed-loop sequences fed
their own answers, in one call (rnn_amd_dream_sequences); ``train_frames`` runs parrot's trainer over a block of frames,
every frame the target of one generation and the input of the next, in one call (rnn_amd_set_dense_steps_tanh).
``train_automaton`` runs rnnca's trainer over a block of a film of bytes, the trainers' rows gathered on the device, in one
call (rnn_amd_set_automaton_steps).  ``train_windows`` runs gstclassify's trainer over a block of windows of features and
class targets, the reference's update gate decided on the device, in one call (rnn_amd_set_classify_steps, or
rnn_amd_classify_generations with balanced training).
``synthetic_text_np`` is the seeded symbol stream of
SURVEY.md section 8(d)'s data-free workload, restated in numpy (Jenkins PRNG, recur-rng.h) so that input data
never comes out of a checker's library.
"""
import ctypes as C

import numpy as np

from . import api as rc



def synthetic_text_np(n=6000, alphabet=42, seed=7):
    """The seeded symbol stream of scenarios.synthetic_text, restated in numpy so
    that fixtures do not depend on any C library (Jenkins PRNG, recur-rng.h)."""
    M = (1 << 64) - 1

    def rot(x, k):
        return ((x << k) | (x >> (64 - k))) & M

    a, b, c, d = 0xF1EA5EED, seed, seed, seed

    def step():
        nonlocal a, b, c, d
        e = (a - rot(b, 7)) & M
        a = b ^ rot(c, 13)
        b = (c + rot(d, 37)) & M
        c = (d + e) & M
        d = (e + a) & M
        return d

    for _ in range(20):
        step()
    out = np.empty(n, np.uint8)
    for i in range(n):
        bits = (step() & 0x000FFFFFFFFFFFFF) | 0x3FF0000000000000
        x = np.frombuffer(np.uint64(bits).tobytes(), dtype=np.float64)[0] - 1.0
        out[i] = int(x * alphabet)
    return out



def text_pointers(texts):
    """(arrays kept alive, u8 *const *texts, int *lens) for a list of numpy uint8 arrays."""
    keep = [np.ascontiguousarray(t, dtype=np.uint8) for t in texts]
    ptrs = (rc.c_u8_p * max(len(keep), 1))(*[rc.u8ptr(t) if len(t) else None for t in keep])
    lens = np.array([len(t) for t in keep], np.int32)
    return keep, ptrs, lens


def run_texts(lib, net, texts, skips=None, alphabet_len=0):
    """rnn_amd_run_texts for a list of numpy uint8 arrays: the array of their sums of log2 p, each text scored on its
    own from the net's current hidden state.  With alphabet_len the net's output row is heads of that many symbols
    (rnn_amd_run_texts_heads) and the result is [len(texts)][heads]."""
    keep, ptrs, lens = text_pointers(texts)
    sk = None if skips is None else np.ascontiguousarray(skips, dtype=np.int32)
    assert sk is None or len(sk) == len(keep)
    heads = net.contents.output_size // alphabet_len if alphabet_len else 1
    sums = np.full((len(keep), heads), np.nan)
    out = sums.ctypes.data_as(C.POINTER(C.c_double))
    skp = None if sk is None else rc.iptr(sk)
    if alphabet_len:
        r = lib.rnn_amd_run_texts_heads(net, ptrs, rc.iptr(lens), skp, len(keep), alphabet_len, out)
    else:
        r = lib.rnn_amd_run_texts(net, ptrs, rc.iptr(lens), skp, len(keep), out)
    if r != 0:
        raise ValueError("rnn_amd_run_texts refused the batch (see stderr)")
    return sums if alphabet_len else sums[:, 0]


TRACE_GUARD = 4  # guard entries behind every array trace_texts hands to the library


def trace_texts(lib, net, texts, alphabet_len=0, guesses=True):
    """rnn_amd_trace_texts for a list of numpy uint8 arrays: per text (logp [len - 1][heads] float32, guess [len - 1][heads]
    uint8 or None), the log2 likelihood of every next symbol and the net's best guess at it, each text on its own from
    the net's current hidden state.  A text shorter than 2 symbols gets empty arrays.  Every array is allocated with
    guard entries behind it (NaN, 0xEE), which must come back untouched."""
    keep, ptrs, lens = text_pointers(texts)
    heads = net.contents.output_size // alphabet_len if alphabet_len else 1
    n = len(keep)
    counts = [max(len(t) - 1, 0) * heads for t in keep]
    lp = [np.full(c + TRACE_GUARD, np.nan, np.float32) for c in counts]
    gs = [np.full(c + TRACE_GUARD, 0xEE, np.uint8) for c in counts] if guesses else None
    lpp = (rc.c_float_p * max(n, 1))(*[rc.fptr(a) for a in lp])
    gsp = (rc.c_u8_p * max(n, 1))(*[rc.u8ptr(a) for a in gs]) if guesses else None
    r = lib.rnn_amd_trace_texts(net, ptrs, rc.iptr(lens), n, alphabet_len, lpp, gsp)
    if r != 0:
        raise ValueError("rnn_amd_trace_texts refused the batch (see stderr)")
    assert all(np.all(np.isnan(a[c:])) for a, c in zip(lp, counts)), "log2 likelihoods behind a text's trace"
    assert all(not np.any(np.isnan(a[:c])) for a, c in zip(lp, counts)), "a traced step was not written"
    assert not guesses or all(np.all(a[c:] == 0xEE) for a, c in zip(gs, counts)), "guesses behind a text's trace"
    return [(lp[k][:counts[k]].reshape(-1, heads).copy(),
             gs[k][:counts[k]].reshape(-1, heads).copy() if guesses else None) for k in range(n)]


def sample_texts(lib, net, first, seeds, max_len, bias=0.0, stop=-1, alphabet_len=0, head=0):
    """rnn_amd_sample_texts: len(first) texts of up to max_len symbols drawn from one net in one batched call, text k from
    symbol first[k] with a generator seeded seeds[k].  Returns (the list of uint8 arrays, the generators afterwards as a
    uint64 array [len(first)][4])."""
    fst = np.ascontiguousarray(first, dtype=np.int32)
    sd = np.ascontiguousarray(seeds, dtype=np.uint64)
    n = len(fst)
    assert len(sd) == n
    out = np.full((max(n, 1), max(max_len, 1)), 0xEE, np.uint8)
    lens = np.full(max(n, 1), -1, np.int32)
    rng = np.zeros((max(n, 1), 4), np.uint64)
    r = lib.rnn_amd_sample_texts(net, rc.iptr(fst), sd.ctypes.data_as(C.POINTER(C.c_uint64)), n, max_len, bias, stop,
                                 alphabet_len, head, rc.u8ptr(out), rc.iptr(lens), rng.ctypes.data_as(C.POINTER(rc.RandCtx)))
    if r != 0:
        raise ValueError("rnn_amd_sample_texts refused the batch or a draw failed (see stderr)")
    assert all(np.all(out[k, lens[k]:max_len] == 0xEE) for k in range(n)), "symbols behind a text's length"
    return [out[k, :lens[k]].copy() for k in range(n)], rng[:n]


def continue_texts(lib, net, prompts, seeds, max_len, bias=0.0, stop=-1, alphabet_len=0, head=0):
    """rnn_amd_continue_texts: the prompts (a list of numpy uint8 arrays) continued by up to max_len symbols each from one
    net in one batched call, continuation k drawn with a generator seeded seeds[k].  Returns what sample_texts returns:
    (the list of uint8 arrays -- the continuations, without their prompts --, the generators afterwards as a uint64
    array [len(prompts)][4])."""
    keep, ptrs, plens = text_pointers(prompts)
    sd = np.ascontiguousarray(seeds, dtype=np.uint64)
    n = len(keep)
    assert len(sd) == n
    out = np.full((max(n, 1), max(max_len, 1)), 0xEE, np.uint8)
    lens = np.full(max(n, 1), -1, np.int32)
    rng = np.zeros((max(n, 1), 4), np.uint64)
    r = lib.rnn_amd_continue_texts(net, ptrs, rc.iptr(plens), sd.ctypes.data_as(C.POINTER(C.c_uint64)), n, max_len, bias,
                                   stop, alphabet_len, head, rc.u8ptr(out), rc.iptr(lens),
                                   rng.ctypes.data_as(C.POINTER(rc.RandCtx)))
    if r != 0:
        raise ValueError("rnn_amd_continue_texts refused the batch or a draw failed (see stderr)")
    assert all(np.all(out[k, lens[k]:max_len] == 0xEE) for k in range(n)), "symbols behind a text's length"
    return [out[k, :lens[k]].copy() for k in range(n)], rng[:n]


def _states(net, n, h_in, want_out, in_place):
    """(h_in array or None, h_out array or None, their pointers) for the _from drivers: states are [n][h_size] float32"""
    H = net.contents.h_size
    hin = None
    if h_in is not None:
        hin = h_in if in_place else np.ascontiguousarray(h_in, dtype=np.float32)
        assert hin.dtype == np.float32 and hin.flags.c_contiguous and hin.shape == (n, H), "states are [n][h_size] float32"
    if in_place:
        assert hin is not None, "an update in place needs h_in"
        hout = hin
    else:
        hout = np.full((max(n, 1), H), np.nan, np.float32) if want_out else None
    return hin, hout, None if hin is None else rc.fptr(hin), None if hout is None else rc.fptr(hout)


def run_texts_from(lib, net, texts, skips=None, alphabet_len=0, h_in=None, want_out=True, in_place=False, sums=True):
    """rnn_amd_run_texts_from: run_texts with a start state per text (h_in [n][h_size] float32, None: the net's hidden
    row) and the texts' final states handed back.  Returns (sums as run_texts returns them, or None with sums=False: the
    texts are fed and nothing is scored; h_out [n][h_size] float32, or None with want_out=False).  in_place: h_out IS the
    caller's h_in array, updated where it lies."""
    keep, ptrs, lens = text_pointers(texts)
    n = len(keep)
    sk = None if skips is None else np.ascontiguousarray(skips, dtype=np.int32)
    assert sk is None or len(sk) == n
    heads = net.contents.output_size // alphabet_len if alphabet_len else 1
    got = np.full((n, heads), np.nan) if sums else None
    hin, hout, hip, hop = _states(net, n, h_in, want_out, in_place)
    r = lib.rnn_amd_run_texts_from(net, ptrs, rc.iptr(lens), None if sk is None else rc.iptr(sk), n, alphabet_len, hip, hop,
                                   got.ctypes.data_as(C.POINTER(C.c_double)) if sums else None)
    if r != 0:
        raise ValueError("rnn_amd_run_texts_from refused the batch (see stderr)")
    if got is not None and not alphabet_len:
        got = got[:, 0]
    return got, None if hout is None else hout[:n]


def trace_texts_from(lib, net, texts, alphabet_len=0, guesses=True, h_in=None, want_out=True, in_place=False):
    """rnn_amd_trace_texts_from: trace_texts with a start state per text and the final states handed back.  Returns (what
    trace_texts returns, h_out [n][h_size] float32 or None)."""
    keep, ptrs, lens = text_pointers(texts)
    heads = net.contents.output_size // alphabet_len if alphabet_len else 1
    n = len(keep)
    counts = [max(len(t) - 1, 0) * heads for t in keep]
    lp = [np.full(c + TRACE_GUARD, np.nan, np.float32) for c in counts]
    gs = [np.full(c + TRACE_GUARD, 0xEE, np.uint8) for c in counts] if guesses else None
    lpp = (rc.c_float_p * max(n, 1))(*[rc.fptr(a) for a in lp])
    gsp = (rc.c_u8_p * max(n, 1))(*[rc.u8ptr(a) for a in gs]) if guesses else None
    hin, hout, hip, hop = _states(net, n, h_in, want_out, in_place)
    r = lib.rnn_amd_trace_texts_from(net, ptrs, rc.iptr(lens), n, alphabet_len, hip, hop, lpp, gsp)
    if r != 0:
        raise ValueError("rnn_amd_trace_texts_from refused the batch (see stderr)")
    assert all(np.all(np.isnan(a[c:])) for a, c in zip(lp, counts)), "log2 likelihoods behind a text's trace"
    assert all(not np.any(np.isnan(a[:c])) for a, c in zip(lp, counts)), "a traced step was not written"
    assert not guesses or all(np.all(a[c:] == 0xEE) for a, c in zip(gs, counts)), "guesses behind a text's trace"
    return [(lp[k][:counts[k]].reshape(-1, heads).copy(),
             gs[k][:counts[k]].reshape(-1, heads).copy() if guesses else None) for k in range(n)], \
        None if hout is None else hout[:n]


def continue_texts_from(lib, net, prompts, seeds, max_len, bias=0.0, stop=-1, alphabet_len=0, head=0, h_in=None, rng_in=None,
                        want_out=True, in_place=False):
    """rnn_amd_continue_texts_from: continue_texts with a start state per prompt (h_in) and, with rng_in (a uint64 array
    [n][4] as the drivers return generators; seeds may then be None), a start generator per prompt; the final states are
    handed back.  Returns (the continuations, the generators afterwards, h_out [n][h_size] float32 or None)."""
    keep, ptrs, plens = text_pointers(prompts)
    n = len(keep)
    sd = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64)
    gi = None if rng_in is None else np.ascontiguousarray(rng_in, dtype=np.uint64)
    assert sd is None or len(sd) == n
    assert gi is None or gi.shape == (n, 4)
    out = np.full((max(n, 1), max(max_len, 1)), 0xEE, np.uint8)
    lens = np.full(max(n, 1), -1, np.int32)
    rng = np.zeros((max(n, 1), 4), np.uint64)
    hin, hout, hip, hop = _states(net, n, h_in, want_out, in_place)
    r = lib.rnn_amd_continue_texts_from(net, ptrs, rc.iptr(plens),
                                        None if sd is None else sd.ctypes.data_as(C.POINTER(C.c_uint64)),
                                        None if gi is None else gi.ctypes.data_as(C.POINTER(rc.RandCtx)), n, max_len, bias,
                                        stop, alphabet_len, head, hip, hop, rc.u8ptr(out), rc.iptr(lens),
                                        rng.ctypes.data_as(C.POINTER(rc.RandCtx)))
    if r != 0:
        raise ValueError("rnn_amd_continue_texts_from refused the batch or a draw failed (see stderr)")
    assert all(np.all(out[k, lens[k]:max_len] == 0xEE) for k in range(n)), "symbols behind a text's length"
    return [out[k, :lens[k]].copy() for k in range(n)], rng[:n], None if hout is None else hout[:n]


def run_sequences(lib, net, seqs, groups=None, h_in=None, want_out=True, in_place=False, segment_frames=0, winners=True):
    """rnn_amd_run_sequences for a list of float32 arrays [frames][input_size] (a sequence may have no frame): per
    sequence (answers [frames][output_size] float32, winners [frames][n_groups] uint8 or None) and h_out [n][h_size]
    float32 (None with want_out=False).  groups: a list of (offset, size) class groups, None or empty for the raw outputs
    (no winners then).  h_in, want_out, in_place as in the _from text drivers.  Every array is allocated with guard
    entries behind it (NaN, 0xEE), which must come back untouched, and every entry in front of them must be written."""
    n = len(seqs)
    isz, osz = net.contents.input_size, net.contents.output_size
    keep = [np.ascontiguousarray(s, dtype=np.float32).reshape(-1, isz) for s in seqs]
    frames = np.array([len(s) for s in keep], np.int32)
    groups = list(groups or [])
    ng = len(groups)
    winners = winners and ng > 0
    goff = np.array([g[0] for g in groups], np.int32)
    gsize = np.array([g[1] for g in groups], np.int32)
    ans = [np.full(int(f) * osz + TRACE_GUARD, np.nan, np.float32) for f in frames]
    win = [np.full(int(f) * ng + TRACE_GUARD, 0xEE, np.uint8) for f in frames] if winners else None
    inp = (rc.c_float_p * max(n, 1))(*[rc.fptr(s) if len(s) else None for s in keep])
    ansp = (rc.c_float_p * max(n, 1))(*[rc.fptr(a) for a in ans])
    winp = (rc.c_u8_p * max(n, 1))(*[rc.u8ptr(a) for a in win]) if winners else None
    hin, hout, hip, hop = _states(net, n, h_in, want_out, in_place)
    r = lib.rnn_amd_run_sequences(net, inp, rc.iptr(frames), n, isz, ng, rc.iptr(goff) if ng else None,
                                  rc.iptr(gsize) if ng else None, hip, hop, segment_frames, ansp, winp)
    if r != 0:
        raise ValueError("rnn_amd_run_sequences refused the batch (see stderr)")
    counts = [int(f) * osz for f in frames]
    assert all(np.all(np.isnan(a[c:])) for a, c in zip(ans, counts)), "answers behind a sequence's last frame"
    assert all(not np.any(np.isnan(a[:c])) for a, c in zip(ans, counts)), "an answer was not written"
    assert not winners or all(np.all(a[int(f) * ng:] == 0xEE) for a, f in zip(win, frames)), "winners behind a sequence's last frame"
    return [(ans[k][:counts[k]].reshape(-1, osz).copy(),
             win[k][:int(frames[k]) * ng].reshape(-1, ng).copy() if winners else None) for k in range(n)], \
        None if hout is None else hout[:n]


def classify_texts(lib, net, texts, skips=None, classes=None, h_in=None, want_out=True, in_place=False):
    """rnn_amd_classify_texts for a list of numpy uint8 arrays (a text may be empty): every symbol fed and, from the
    text's skip on, the softmax over all outputs added up.  classes: None, or a list with, per text, None or a uint8 array
    of the text's length (0xFF: the symbol has no class).  Returns (sums [n][output_size] float64, sumsqs the same,
    scores as a structured array [n] with fields error, entropy (float64), correct, count (int64), h_out [n][h_size]
    float32 or None with want_out=False).  h_in, want_out, in_place as in the _from text drivers.  The result arrays are
    allocated with guard entries behind them, which must come back untouched."""
    keep, ptrs, lens = text_pointers(texts)
    n = len(keep)
    osz = net.contents.output_size
    sk = None if skips is None else np.ascontiguousarray(skips, dtype=np.int32)
    assert sk is None or len(sk) == n
    ckeep, cptrs = None, None
    if classes is not None:
        assert len(classes) == n
        ckeep = [None if c is None else np.ascontiguousarray(c, dtype=np.uint8) for c in classes]
        assert all(c is None or len(c) == len(t) for c, t in zip(ckeep, keep)), "a class byte per symbol"
        cptrs = (rc.c_u8_p * max(n, 1))(*[rc.u8ptr(c) if c is not None and len(c) else None for c in ckeep])
    sums = np.full(n * osz + TRACE_GUARD, np.nan)
    sumsqs = np.full(n * osz + TRACE_GUARD, np.nan)
    scores = np.full(n + 1, -7, np.dtype([("error", np.float64), ("entropy", np.float64), ("correct", np.int64),
                                          ("count", np.int64)]))
    assert scores.dtype.itemsize == C.sizeof(rc.ClassScore)
    hin, hout, hip, hop = _states(net, n, h_in, want_out, in_place)
    dp = C.POINTER(C.c_double)
    r = lib.rnn_amd_classify_texts(net, ptrs, rc.iptr(lens), None if sk is None else rc.iptr(sk), cptrs, n, hip, hop,
                                   sums.ctypes.data_as(dp), sumsqs.ctypes.data_as(dp),
                                   scores.ctypes.data_as(C.POINTER(rc.ClassScore)))
    if r != 0:
        raise ValueError("rnn_amd_classify_texts refused the batch (see stderr)")
    assert np.all(np.isnan(sums[n * osz:])) and np.all(np.isnan(sumsqs[n * osz:])), "sums behind the last text's"
    assert scores[n]["count"] == -7 and scores[n]["error"] == -7, "a score behind the last text's"
    assert not np.any(np.isnan(sums[:n * osz])) and not np.any(np.isnan(sumsqs[:n * osz])), "a sum was not written"
    return sums[:n * osz].reshape(n, osz).copy(), sumsqs[:n * osz].reshape(n, osz).copy(), scores[:n].copy(), \
        None if hout is None else hout[:n]


def parse_offsets(lib, pattern, max_pairs=512):
    """rnn_amd_automaton_parse_offsets: (the Y offsets, the C offsets) of an rnnca offset pattern such as
    "Y00120111C0111", as int32 arrays [n][2] of (dx, dy).  The arrays are allocated with guard entries behind them, which
    must come back untouched."""
    oy = np.full(2 * max_pairs + TRACE_GUARD, -77, np.int32)
    oc = np.full(2 * max_pairs + TRACE_GUARD, -77, np.int32)
    ny, nc = C.c_int(-1), C.c_int(-1)
    r = lib.rnn_amd_automaton_parse_offsets(pattern.encode() if isinstance(pattern, str) else pattern, rc.iptr(oy),
                                            C.byref(ny), rc.iptr(oc), C.byref(nc), max_pairs)
    assert np.all(oy[2 * max_pairs:] == -77) and np.all(oc[2 * max_pairs:] == -77), "offsets behind an array's room"
    if r != 0:
        raise ValueError("rnn_amd_automaton_parse_offsets refused the pattern (see stderr)")
    assert np.all(oy[2 * ny.value:] == -77) and np.all(oc[2 * nc.value:] == -77), "offsets behind a list's length"
    return oy[:2 * ny.value].reshape(-1, 2).copy(), oc[:2 * nc.value].reshape(-1, 2).copy()


class AutomatonGeometry:
    """an RnnAmdAutomaton and the arrays it points at: a width x height grid, the (dx, dy) offset lists [n][2], two or
    three position inputs, clamped (edges != 0) or once-wrapped edges"""

    def __init__(self, width, height, offsets_y, offsets_c, len_pos=2, edges=1):
        self.width, self.height, self.len_pos, self.edges = width, height, len_pos, edges
        self.offsets_y = np.ascontiguousarray(offsets_y, dtype=np.int32).reshape(-1, 2)
        self.offsets_c = np.ascontiguousarray(offsets_c, dtype=np.int32).reshape(-1, 2)
        self.input_size = len(self.offsets_y) + 2 * len(self.offsets_c) + len_pos
        self.struct = rc.Automaton(width, height, rc.iptr(self.offsets_y) if len(self.offsets_y) else None,
                                   len(self.offsets_y), rc.iptr(self.offsets_c) if len(self.offsets_c) else None,
                                   len(self.offsets_c), len_pos, edges)


def run_automaton(lib, net, geometry, seed, n_frames, h_in=None, want_out=True, in_place=False, segment_frames=0, fill=0xEE):
    """rnn_amd_run_automaton: n_frames frames of rnnca's automaton on the grid of `geometry` (an AutomatonGeometry) from
    the seed frame (uint8 [3][height][width]), every cell a forward-only clone of net.  Returns (frames uint8
    [n_frames][3][height][width], h_out [cells][h_size] float32 or None with want_out=False).  h_in (None: the net's
    hidden row), want_out and in_place as in the _from text drivers.  Every array is allocated with guard bytes behind it
    (`fill`, NaN), which must come back untouched, and every state in front of them must be written; that every byte of
    the frames is written shows in two calls with different `fill` giving the same frames."""
    g = geometry
    cells, H = g.width * g.height, net.contents.h_size
    sd = np.ascontiguousarray(seed, dtype=np.uint8)
    assert sd.size == 3 * cells, "a seed frame is [3][height][width] bytes"
    count = n_frames * 3 * cells
    frames = np.full(count + TRACE_GUARD, fill, np.uint8)
    hin, hout, hip, _ = _states(net, cells, h_in, False, in_place)
    if want_out and not in_place:
        hout = np.full((cells + 1, H), np.nan, np.float32)   # (a guard row behind the states)
    r = lib.rnn_amd_run_automaton(net, C.byref(g.struct), rc.u8ptr(sd), n_frames, hip, None if hout is None else rc.fptr(hout),
                                  segment_frames, rc.u8ptr(frames))
    if r != 0:
        raise ValueError("rnn_amd_run_automaton refused the call (see stderr)")
    assert np.all(frames[count:] == fill), "bytes behind the last frame"
    if hout is not None and not in_place:
        assert np.all(np.isnan(hout[cells])), "floats behind the last state"
        hout = hout[:cells]
        assert not np.any(np.isnan(hout[:, 1:1 + net.contents.hidden_size])), "a state was not written"
    return frames[:count].reshape(n_frames, 3, g.height, g.width).copy(), hout


def dream_sequences(lib, net, first, n_frames, noise=1.0, seeds=None, rng_in=None, h_in=None, segment_frames=0,
                    want_out=True, in_place=False):
    """rnn_amd_dream_sequences: n_frames frames of parrot's player for len(first) closed-loop sequences, every sequence a
    forward-only clone of net fed its own last answer, from the rows of first (float32 [n][ld], ld >= input_size).
    seeds: a uint64 per sequence; rng_in: a uint64 array [n][4] as the drivers return generators (seeds may then be
    None); with noise == 0 both may be None.  Returns (frames float32 [n_frames][n][output_size], next float32
    [n][input_size], h_out [n][h_size] float32 or None with want_out=False, rng_out uint64 [n][4]).  h_in, want_out and
    in_place as in the _from text drivers; in_place also hands rng_in itself to the call as rng_out.  frames and next are
    allocated with guard floats behind them (NaN), which must come back untouched."""
    fr = np.ascontiguousarray(first, dtype=np.float32)
    assert fr.ndim == 2, "first is [n][ld]"
    n, ld = fr.shape
    isz, osz = net.contents.input_size, net.contents.output_size
    sd = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64)
    assert sd is None or len(sd) == n
    gi = None
    if rng_in is not None:
        gi = rng_in if in_place else np.ascontiguousarray(rng_in, dtype=np.uint64)
        assert gi.dtype == np.uint64 and gi.flags.c_contiguous and gi.shape == (n, 4), "generators are [n][4] uint64"
    count = n_frames * n * osz
    frames = np.full(count + TRACE_GUARD, np.nan, np.float32)
    nxt = np.full(n * isz + TRACE_GUARD, np.nan, np.float32)
    rng = gi if in_place and gi is not None else np.zeros((max(n, 1), 4), np.uint64)
    hin, hout, hip, hop = _states(net, n, h_in, want_out, in_place)
    r = lib.rnn_amd_dream_sequences(net, rc.fptr(fr), ld, n, n_frames, noise,
                                    None if sd is None else sd.ctypes.data_as(C.POINTER(C.c_uint64)),
                                    None if gi is None else gi.ctypes.data_as(C.POINTER(rc.RandCtx)), hip, hop,
                                    segment_frames, rc.fptr(frames), rc.fptr(nxt), rng.ctypes.data_as(C.POINTER(rc.RandCtx)))
    if r != 0:
        raise ValueError("rnn_amd_dream_sequences refused the call (see stderr)")
    assert np.all(np.isnan(frames[count:])) and np.all(np.isnan(nxt[n * isz:])), "floats behind the last frame or row"
    return frames[:count].reshape(n_frames, n, osz).copy(), nxt[:n * isz].reshape(n, isz).copy(), \
        None if hout is None else hout[:n], rng[:n]


def train_frames(lib, set_or_handle, frames, n, learning_style=rc.WEIGHTED, momentum=0.95, condition=False):
    """rnn_amd_set_dense_steps_tanh: parrot's trainer over a block of frames, float32 [T + 1][n_nets][ld] with
    ld >= max(input_size, n): T generations in one call, generation t fed frames[t] and scored against the first n values
    of frames[t + 1] (tanh answer, slope error, the deltas summed over the nets, the update; rnn_condition_net behind
    each with condition).  set_or_handle: an AmdBatchedSet or an RnnAmdSet handle.  The last frame of a block is the first
    of the next.  Returns T."""
    handle = getattr(set_or_handle, "handle", set_or_handle)
    fr = np.ascontiguousarray(frames, dtype=np.float32)
    assert fr.ndim == 3 and fr.shape[0] >= 2, "frames are [T + 1][n_nets][ld], T >= 1"
    assert fr.shape[1] == lib.rnn_amd_set_size(handle), "one row per net of the set in every frame"
    lib.rnn_amd_set_dense_steps_tanh(handle, rc.fptr(fr), fr.shape[2], fr.shape[0] - 1, n, learning_style, momentum,
                                     int(bool(condition)))
    return fr.shape[0] - 1


def train_automaton(lib, set_or_handle, geometry, frames, xy, advance=False, learning_style=rc.WEIGHTED, momentum=0.95,
                    soft_start=0.0, condition=False):
    """rnn_amd_set_automaton_steps: rnnca's trainer over a block of a film, uint8 [T + 1][3][height][width] on the grid of
    `geometry` (an AutomatonGeometry): T generations in one call, generation t's trainers fed fill_net_inputs of frames[t]
    at their cells and scored against the three bytes of frames[t + 1] there (sigmoid answer, slope error, the deltas summed
    over the trainers, the update with the soft-started momentum; rnn_condition_net behind each with condition).  xy: the
    trainers' (x, y), int32 [n][2] for the whole block or [T][n][2], a list per generation.  advance: rnn_bptt_advance in
    front of every opinion (the plugin does not).  set_or_handle: an AmdBatchedSet or an RnnAmdSet handle.  The last frame
    of a block is the first of the next.  Returns T."""
    handle = getattr(set_or_handle, "handle", set_or_handle)
    g = geometry
    fr = np.ascontiguousarray(frames, dtype=np.uint8)
    assert fr.ndim == 4 and fr.shape[0] >= 2 and fr.shape[1:] == (3, g.height, g.width), "frames are [T + 1][3][height][width]"
    T = fr.shape[0] - 1
    pos = np.ascontiguousarray(xy, dtype=np.int32)
    n = lib.rnn_amd_set_size(handle)
    assert pos.shape in ((n, 2), (T, n, 2)), "xy is [n][2] or [T][n][2], n the nets of the set"
    lib.rnn_amd_set_automaton_steps(handle, C.byref(g.struct), rc.u8ptr(fr), rc.iptr(pos), int(pos.ndim == 3), T,
                                    int(bool(advance)), learning_style, momentum, soft_start, int(bool(condition)))
    return T


def train_windows(lib, set_or_handle, features, targets, group_offset, group_size, error_weight=None, balance=None,
                  learning_style=rc.NESTEROV, soft_start=2000.0, condition=True):
    """rnn_amd_set_classify_steps: gstclassify's trainer (maybe_learn) over a block of windows in one call.  features:
    float32 [T][n][ld], ld >= the net's inputs; targets: int32 [T][n][G], the class of channel j in group i at window t, < 0
    or >= the group's size for "no label"; group_offset / group_size: the G class groups' first output and size;
    error_weight: a factor per output, or None.  Generation t clears the deltas, forms every channel's opinion of
    features[t], the class-group loss against targets[t], the deltas of the labelled channels, advances the rings, updates
    with the soft-started momentum if the generation's summed error is not zero (the reference's `if (err_sum)`, decided on
    the device) and conditions the net when `condition`.  balance: a pointer from rnn_amd_balanced_new; then the call is
    rnn_amd_classify_generations (the library bound with bind_classify), which draws every generation's balanced sample
    ahead and always conditions.  set_or_handle: an AmdBatchedSet or an RnnAmdSet handle.  Returns the number of groups
    trained (with balance: the library's count; otherwise counted here from the targets)."""
    handle = getattr(set_or_handle, "handle", set_or_handle)
    x = np.ascontiguousarray(features, dtype=np.float32)
    tg = np.ascontiguousarray(targets, dtype=np.int32)
    goff = np.ascontiguousarray(group_offset, dtype=np.int32)
    gsize = np.ascontiguousarray(group_size, dtype=np.int32)
    n = lib.rnn_amd_set_size(handle)
    assert x.ndim == 3 and x.shape[0] >= 1 and x.shape[1] == n, "features are [T][n][ld], n the nets of the set"
    assert goff.ndim == 1 and goff.shape == gsize.shape and len(goff) >= 1, "one offset and one size per class group"
    assert tg.shape == (x.shape[0], n, len(goff)), "targets are [T][n][G]"
    w = None if error_weight is None else np.ascontiguousarray(error_weight, dtype=np.float32)
    wp = None if w is None else rc.fptr(w)
    if balance is not None:
        assert condition, "rnn_amd_classify_generations always conditions the net"
        return lib.rnn_amd_classify_generations(handle, rc.fptr(x), x.shape[2], rc.iptr(tg), x.shape[0], len(goff), rc.iptr(goff),
                                                rc.iptr(gsize), wp, balance, learning_style, soft_start)
    lib.rnn_amd_set_classify_steps(handle, rc.fptr(x), x.shape[2], rc.iptr(tg), x.shape[0], len(goff), rc.iptr(goff),
                                   rc.iptr(gsize), wp, learning_style, soft_start, int(bool(condition)))
    return int(((tg >= 0) & (tg < gsize[None, None, :])).sum())


class ApiSet:
    """A training set held by an rnn_* library (reference or product)."""

    def __init__(self, lib, input_size, hidden_size, output_size, S, D, activation=rc.RELU,
                 flags=rc.FLAG_STANDARD | rc.FLAG_ADAPTIVE_MIN_ERROR, learn_rate=1e-3, seed=1,
                 momentum=0.95, variance=None, shape=rc.DIST_SEMICIRCLE, perforation=0.0,
                 softmax_best_guess=None, noise=0.0, bottom_inputs=0, bottom_rate_scale=1.0,
                 shard=None):
        self.lib = lib
        self.S, self.D = S, D
        # shard = (global_first, global_count): this set holds S of the streams of a larger
        # logical set (one shard per GPU / process)
        self.global_first, self.global_count = shard if shard else (0, S)
        # with bottom_inputs the net sits on a bottom layer: `input_size` is that
        # layer's output size and bottom_inputs its input size
        # (rnn_new_with_bottom_layer, recur-nn-init.c:194-219)
        self.bottom_inputs = bottom_inputs
        if bottom_inputs:
            net = lib.rnn_new_with_bottom_layer(bottom_inputs, input_size, hidden_size, output_size,
                                                flags, seed, None, D, learn_rate, momentum, noise,
                                                activation, 0)
            net.contents.bottom_layer.contents.learn_rate_scale = bottom_rate_scale
        else:
            net = lib.rnn_new(input_size, hidden_size, output_size, flags, seed, None, D,
                              learn_rate, momentum, noise, activation)
        self.net = net
        n = net.contents
        self.I, self.H, self.O = n.i_size, n.h_size, n.o_size
        self.input_size, self.hidden_size, self.output_size = input_size, hidden_size, output_size
        p = rc.InitParams()
        lib.rnn_init_default_weight_parameters(net, C.byref(p))
        p.method = rc.INIT_FLAT
        if variance is not None:
            p.flat_variance = variance
        p.flat_shape = shape
        p.flat_perforation = perforation
        lib.rnn_randomise_weights_clever(net, C.byref(p))
        if shard and shard != (0, S):
            self.nets = lib.rnn_amd_new_training_set_shard(net, S, shard[0], shard[1])
        else:
            self.nets = lib.rnn_new_training_set(net, S)
        # the caller-side loss (softmax_best_guess is a static inline of the
        # reference's badmaths.h, i.e. caller code, not library code)
        self._sbg = softmax_best_guess

    def close(self):
        self.lib.rnn_delete_training_set(self.nets, self.S, 0)

    # -- per-stream steps (the reference call sequence) --
    def one_hot_opinion(self, j, hot, noise=0.0):
        n = self.nets[j].contents
        if self.bottom_inputs:
            # the helper's bottom-layer branch indexes from the bias slot
            # (charmodel-helpers.h:20-23, 30-31)
            real = rc.view(n.bottom_layer.contents.inputs, self.bottom_inputs)
        else:
            real = rc.view(n.real_inputs, self.input_size)
        real[:] = 0
        real[hot] = 1.0
        return self.lib.rnn_opinion(self.nets[j], None, noise)

    def net_error_bptt(self, j, c, nxt):
        n = self.nets[j].contents
        answer = self.one_hot_opinion(j, c, n.presynaptic_noise)
        err = n.bptt.contents.o_error
        winner = self._sbg(err, answer, self.output_size)
        e = rc.view(err, self.O)
        e[nxt] += 1.0
        return float(e[nxt]), int(winner == nxt)

    def char_step_deltas(self, text, i):
        L = len(text)
        spacing = (L - 1) // self.global_count
        stats = []
        for j in range(self.S):
            off = i + (self.global_first + j) * spacing
            if off >= L - 1:
                off -= L - 1
            self.lib.rnn_bptt_advance(self.nets[j])
            stats.append(self.net_error_bptt(j, int(text[off]), int(text[off + 1])))
            self.lib.rnn_bptt_calc_deltas(self.nets[j], 1 if j else 0, None)
        return stats

    def char_step(self, text, i, method=rc.WEIGHTED, momentum=0.95):
        stats = self.char_step_deltas(text, i)
        self.lib.rnn_apply_learning(self.net, method, momentum)
        return stats

    def sync(self):
        if hasattr(self.lib, "rnn_amd_sync_host"):
            self.lib.rnn_amd_sync_host(self.net, rc.RNN_AMD_EVERYTHING)

    def snapshot(self):
        self.sync()
        n0 = self.net.contents
        b0 = n0.bptt.contents
        S, D, I, H, O = self.S, self.D, self.I, self.H, self.O
        snap = {
            "ih_w": rc.view(n0.ih_weights, I, H).copy(),
            "ho_w": rc.view(n0.ho_weights, H, O).copy(),
            "ih_m": rc.view(b0.ih_momentum, I, H).copy(),
            "ho_m": rc.view(b0.ho_momentum, H, O).copy(),
            "ih_delta": rc.view(b0.ih_delta, I, H).copy(),
            "ho_delta": rc.view(b0.ho_delta, H, O).copy(),
        }
        if self.bottom_inputs:
            bl = n0.bottom_layer.contents
            snap.update(b_w=rc.view(bl.weights, bl.i_size, bl.o_size).copy(),
                        b_m=rc.view(bl.momentums, bl.i_size, bl.o_size).copy(),
                        b_delta=rc.view(bl.delta, bl.i_size, bl.o_size).copy(),
                        b_o_error=rc.view(bl.o_error, bl.o_size).copy())
        hist = np.zeros((D, S, I), np.float32)
        hidden = np.zeros((S, H), np.float32)
        output = np.zeros((S, O), np.float32)
        o_error = np.zeros((S, O), np.float32)
        index = np.zeros(S, np.int32)
        mef = np.zeros(S, np.float32)
        ih_scale = np.zeros(S, np.float32)
        gen = np.zeros(S, np.uint32)
        rng = np.zeros((S, 4), np.uint64)
        for j in range(S):
            n = self.nets[j].contents
            b = n.bptt.contents
            hist[:, j, :] = rc.view(b.history, D, I)
            hidden[j] = rc.view(n.hidden_layer, H)
            output[j] = rc.view(n.output_layer, O)
            o_error[j] = rc.view(b.o_error, O)
            index[j] = b.index
            mef[j] = b.min_error_factor
            ih_scale[j] = b.ih_scale
            gen[j] = n.generation
            rng[j] = (n.rng.a, n.rng.b, n.rng.c, n.rng.d)
        snap.update(hist=hist, hidden=hidden, output=output, o_error=o_error, index=index,
                    min_error_factor=mef, ih_scale=ih_scale, generation=gen, rng=rng)
        return snap


class AmdBatchedSet(ApiSet):
    """librecur_amd.so driven through its additive batched entry points
    (include/recur_amd.h part 2): the whole set per call, text on the device."""

    def __init__(self, lib, *args, **kw):
        super().__init__(lib, *args, **kw)
        self.handle = lib.rnn_amd_set_open(self.nets, self.S)
        assert self.handle, "rnn_amd_set_open failed"
        self._text = None

    def load_text(self, text):
        self._text = np.ascontiguousarray(text, dtype=np.uint8)
        self.lib.rnn_amd_set_load_text(self.handle, rc.u8ptr(self._text), len(self._text))

    def char_step_deltas(self, text, i):
        if self._text is None or self._text is not text:
            self.load_text(text)
        self.lib.rnn_amd_set_char_step_deltas(self.handle, i)

    def char_step(self, text, i, method=rc.WEIGHTED, momentum=0.95):
        if self._text is None or (self._text is not text and not np.array_equal(self._text, text)):
            self.load_text(text)
        self.lib.rnn_amd_set_char_step(self.handle, i, method, momentum)

    def stats(self, clear=False):
        st = rc.AmdStats()
        self.lib.rnn_amd_set_read_stats(self.handle, C.byref(st), int(clear))
        return st

    def close(self):
        self.lib.rnn_amd_set_close(self.handle)
        super().close()
