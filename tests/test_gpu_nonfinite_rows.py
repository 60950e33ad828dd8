"""Every loss and scoring kernel of the device on output rows that are NOT finite: an infinity or a NaN among the logits
(loss_edge_cases.nonfinite_rows), produced on the device from finite written weights (designed_nonfinite_weights: one
product overflows).  The reference's fast_expf does not return on an infinity, so there is no oracle here -- the oracle
restates the reference and must never see such a row.  What is held is the library's own contract (include/recur_amd.h,
"Rows that are not finite"), by running every case TWICE on fresh nets: the poisoned run, in which about five of twelve
streams or texts select a row that is not finite, and the control run, the same call with those symbols replaced by the
`plain` row's symbol (same shapes, same plans).  Where a call walks a text and scores every symbol against the next one
(the cross entropies, rnn_amd_run_texts and _heads, rnn_amd_trace_texts) a symbol is also the target of the step before it,
so there the control keeps the text and the poisoned symbols select the plain row in the control's net (`twin`): the
steps around a poisoned one then have the same targets in both runs and are held bit for bit.

  * the call returns;
  * every output row is the written one: finite and infinite elements by their bits, NaN as NaN;
  * on clean streams every float result is the control's, bit for bit;
  * on poisoned streams every float result is NaN over exactly the scored range (the numpy restatement's NaN mask) and
    the control's bits outside it: the other heads, the other class groups, the outputs that take no sigmoid;
  * `count` is exact; `correct` lies between the control's and the control's plus the number of poisoned softmaxes
    (the control's target there is never the best guess; the best guess of a softmax without likelihoods is unspecified);
  * the set-wide sums are NaN in the poisoned run and finite in the control;
  * the hidden rows and the history are the control's on clean streams and the written net's on poisoned ones.
Deltas and weights are not held after a poisoned step (a NaN spreads through their sums): one step per net, then it is
closed.  The CPU half (tests/test_fast_exp_rule.py) shows that each of these rows reaches the exponential's scaling loop
with an infinite argument and that the written weights give exactly these rows.

These tests must never run on a build whose exponential can loop on an infinity (anything before fast_exp_rule.h): there
the kernels do not return."""
import ctypes as C

import numpy as np
import pytest

import loss_edge_cases as le
import recur_ctypes as rc
import scenarios as sc
from recur_amd.drivers import text_pointers

pytestmark = pytest.mark.gpu
F = np.float32
HIDDEN = 64
S = 12
POISONED = (1, 4, 6, 9, 11)          # the streams (texts) that select a row that is not finite
CLEAN = tuple(j for j in range(S) if j not in POISONED)
CLEAN_NAMES = ("plain", "at_50", "limited", "lowered")   # symbol 0 is `plain`: the control's stand-in
SAMPLE_MAX_ATTEMPTS = 64             # sample_rule.h


@pytest.fixture(scope="module")
def amd():
    lib = rc.bind_classify(rc.bind_char(rc.load_amd()))
    assert lib.rnn_amd_device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return lib


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    """bit for bit (float32)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.array_equal(_bits(a), _bits(b)))


def same64(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def is_written(got, row):
    """finite and infinite elements by their bits, NaN as NaN"""
    got, row = np.asarray(got, np.float32), np.asarray(row, np.float32)
    nan = np.isnan(row)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got[~nan]), _bits(row[~nan])))


def symbols(n):
    """-> (names, rows): the clean catalogue rows CLEAN_NAMES, then every row of nonfinite_rows(n)"""
    clean, bad = le.rows(n), le.nonfinite_rows(n)
    names = list(CLEAN_NAMES) + list(bad)
    return names, [clean[k] for k in CLEAN_NAMES] + [bad[k] for k in bad]


def dealt(n_bad, first=len(CLEAN_NAMES), kinds=None):
    """the symbol of every stream in the poisoned run: the poisoned streams walk the rows that are not finite (`kinds`:
    only those), the clean ones the clean rows.  -> int array [S]"""
    bad = list(range(first, first + n_bad)) if kinds is None else list(kinds)
    sym = np.zeros(S, np.int32)
    for k, j in enumerate(POISONED):
        sym[j] = bad[k % len(bad)]
    for k, j in enumerate(CLEAN):
        sym[j] = k % first
    return sym


def control_of(sym, first=len(CLEAN_NAMES)):
    return np.where(sym >= first, 0, sym).astype(np.int32)


def twin(rows_):
    """the control of the calls that WALK A TEXT and score every symbol against the next one (the cross entropies, the
    scorers, the trace): there a symbol is also the target of the step before it, so putting symbol 0 in its place would
    move that step's likelihood too.  The control keeps the text and is a net in which every row that is not finite is
    the `plain` symbol's row: the poisoned symbols select the plain row, and nothing else changes."""
    return [r if np.isfinite(r).all() else rows_[0] for r in rows_]


def write_weights(lib, net, I, H, O, ih, ho, momentum=True):
    n0 = net.contents
    lib.rnn_amd_sync_host(net, rc.RNN_AMD_EVERYTHING)
    rc.view(n0.ih_weights, I, H)[:] = ih
    rc.view(n0.ho_weights, H, O)[:] = ho
    what = rc.RNN_AMD_WEIGHTS
    if momentum:
        b0 = n0.bptt.contents
        rc.view(b0.ih_momentum, I, H)[:] = 0
        rc.view(b0.ho_momentum, H, O)[:] = 0
        what |= rc.RNN_AMD_MOMENTUMS
    lib.rnn_amd_host_written(net, what)


class Written:
    """a fresh training set whose net is the written one (learn rate 0, zero momentum), and that net on the CPU"""

    def __init__(self, lib, rows_, input_size, output_size, n_streams=S, hidden_size=HIDDEN, D=4, batched=True):
        kw = dict(input_size=input_size, hidden_size=hidden_size, output_size=output_size, S=n_streams, D=D, learn_rate=0.0,
                  seed=3)
        self.lib, self.rows, self.hidden_size = lib, rows_, hidden_size
        self.g = g = (sc.AmdBatchedSet if batched else sc.ApiSet)(lib, **kw)
        self.ih, self.ho = le.designed_nonfinite_weights(g.I, g.H, g.O, hidden_size, rows_)
        write_weights(lib, g.net, g.I, g.H, g.O, self.ih, self.ho)
        snap = g.snapshot()
        assert np.array_equal(snap["ih_w"], self.ih) and np.array_equal(snap["ho_w"], self.ho)

    def hold_rows(self, snap, sym):
        """every stream's output row and hidden row are the written net's answer to its symbol"""
        for j, c in enumerate(sym):
            hid, out = le.designed_forward(self.ih, self.ho, self.hidden_size, int(c))
            row = self.rows[int(c)]
            assert is_written(out[:len(row)], row)                                   # (the CPU half's, once more)
            assert is_written(snap["output"][j, :len(row)], row), "stream %d: the output row is not the written one" % j
            assert same(snap["hidden"][j, :1 + self.hidden_size], hid[:1 + self.hidden_size]), "stream %d: hidden" % j

    def close(self):
        self.g.close()


def hold_streams(p, c, sym, scored, n_out, keys=("o_error",)):
    """p, c: the poisoned and the control run's snapshots.  scored(j) -> bool mask [n_out] of the floats of stream j that
    derive from a softmax (or a sigmoid) that is not finite: NaN there, the control's bits everywhere else; hidden rows and
    history the control's on every clean stream"""
    first = len(CLEAN_NAMES)
    for j in range(len(sym)):
        bad = scored(j)
        assert bad.any() == (sym[j] >= first), j
        for k in keys:
            got, want = p[k][j], c[k][j]
            assert np.isfinite(want).all(), (k, j)
            assert np.array_equal(np.isnan(got[:n_out]), bad), "stream %d: %s is NaN at %s, expected at %s" % (
                j, k, np.nonzero(np.isnan(got[:n_out]))[0], np.nonzero(bad)[0])
            assert same(got[:n_out][~bad], want[:n_out][~bad]), "stream %d: %s differs from the control's" % (j, k)
            assert same(got[n_out:], want[n_out:]), "stream %d: %s behind the outputs" % (j, k)
        if sym[j] < first:
            assert same(p["hidden"][j], c["hidden"][j]) and same(p["hist"][:, j], c["hist"][:, j]), j
            assert same(p["output"][j], c["output"][j]), j


def hold_stats(p, c, n_poisoned, count):
    """the set-wide sums: NaN in the poisoned run, finite in the control; count exact; correct within the bounds"""
    assert p.count == c.count == count
    assert np.isnan(p.error) and np.isfinite(c.error)
    assert c.correct <= p.correct <= c.correct + n_poisoned, (p.correct, c.correct)


def restated_nan(row, target):
    """the numpy restatement's NaN mask of a softmax error row"""
    return np.isnan(le.scored(row, target)["error"])


def far_target(row):
    """a target that is not the row's best guess"""
    return int(np.argmin(np.where(np.isfinite(row), row, np.inf)))


# ------------------------------------------------------------------ the stand-alone loss --

def stand_alone(amd, n, sym, tgt, rows_):
    w = Written(amd, rows_, 24, n)
    g = w.g
    g.stats(clear=True)
    amd.rnn_amd_set_advance(g.handle)
    amd.rnn_amd_set_one_hot_opinion(g.handle, rc.iptr(sym), None)
    amd.rnn_amd_set_softmax_error(g.handle, rc.iptr(tgt))
    amd.rnn_amd_set_calc_deltas(g.handle, 0, None, None)
    snap, st = g.snapshot(), g.stats()
    w.hold_rows(snap, sym)
    w.close()
    return snap, st


@pytest.mark.parametrize("kinds", ["pos_inf", "all"])
@pytest.mark.parametrize("n", [42, 130])
def test_stand_alone_loss(amd, n, kinds):
    """rnn_amd_set_one_hot_opinion + rnn_amd_set_softmax_error + rnn_amd_set_calc_deltas: k_softmax_error, at 42 and, with
    the infinity in a lane's third value, at 130.  (n = 42 with pos_inf alone is the smallest case of the module.)"""
    names, rows_ = symbols(n)
    sym = dealt(len(rows_) - len(CLEAN_NAMES), kinds=[names.index("pos_inf")] if kinds == "pos_inf" else None)
    ctl = control_of(sym)
    tgt = np.array([far_target(rows_[c]) if j in POISONED else (int(np.argmax(rows_[c])), far_target(rows_[c]))[j % 2]
                    for j, c in enumerate(sym)], np.int32)
    assert all(tgt[j] != int(np.argmax(rows_[0])) for j in POISONED)
    p, pst = stand_alone(amd, n, sym, tgt, rows_)
    c, cst = stand_alone(amd, n, ctl, tgt, rows_)
    hold_streams(p, c, sym, lambda j: restated_nan(rows_[sym[j]], tgt[j]) & (sym[j] >= len(CLEAN_NAMES)), n)
    for j in POISONED:
        assert np.isnan(p["o_error"][j, :n]).all()
    hold_stats(pst, cst, len(POISONED), S)
    assert np.isnan(pst.entropy) and np.isfinite(cst.entropy) and 0 < cst.correct < S


# ------------------------------------------------------------------ the text step --

def text_step(amd, n, sym, tgt, rows_):
    w = Written(amd, rows_, n, n)
    g = w.g
    text, positions, plan = le.stream_text([(int(c), int(t)) for c, t in zip(sym, tgt)], S)
    assert positions == [0] and [c for c, _ in plan[0]] == list(sym)
    g.stats(clear=True)
    g.char_step(text, 0, rc.WEIGHTED, 0.9)
    snap, st = g.snapshot(), g.stats()
    w.hold_rows(snap, sym)
    w.close()
    return snap, st


@pytest.mark.parametrize("n", [42, 64, 65, 130])
def test_text_step(amd, n):
    """rnn_amd_set_char_step: k_text_top2 (42; 64, where every lane has a value) and k_text_top<0> (65; 130, the infinity in
    a lane's third value)"""
    names, rows_ = symbols(n)
    sym = dealt(len(rows_) - len(CLEAN_NAMES))
    ctl = control_of(sym)
    tgt = np.array([far_target(rows_[c]) if j in POISONED else (int(np.argmax(rows_[c])), far_target(rows_[c]))[j % 2]
                    for j, c in enumerate(sym)], np.int32)
    p, pst = text_step(amd, n, sym, tgt, rows_)
    c, cst = text_step(amd, n, ctl, tgt, rows_)
    hold_streams(p, c, sym, lambda j: restated_nan(rows_[sym[j]], tgt[j]) & (sym[j] >= len(CLEAN_NAMES)), n)
    hold_stats(pst, cst, len(POISONED), S)
    assert np.isnan(pst.entropy) and np.isfinite(cst.entropy) and 0 < cst.correct < S


# ------------------------------------------------------------------ heads --

def head_symbols(alen, heads):
    """-> (rows [symbol][alen heads], the poisoned head of every symbol or -1): clean symbols hold catalogue rows in every
    head, a poisoned one the `plain` rows of symbol 0 with ONE head replaced by a row that is not finite"""
    clean = [np.concatenate([le.rows(alen, h)[name] for h in range(heads)]) for name in CLEAN_NAMES]
    full, where = list(clean), [-1] * len(clean)
    for k, (name, row) in enumerate(le.nonfinite_rows(alen).items()):
        r = clean[0].copy()
        h = (k + 1) % heads
        r[h * alen:(h + 1) * alen] = np.where(np.isfinite(row), r[h * alen:(h + 1) * alen], row)
        full.append(r)
        where.append(h)
    return full, where


def heads_step(amd, alen, heads, sym, nxt, cls, rows_):
    w = Written(amd, rows_, 16, alen * heads, hidden_size=HIDDEN)
    g = w.g
    g.stats(clear=True)
    amd.rnn_amd_set_multi_step(g.handle, rc.iptr(sym), rc.iptr(nxt), rc.iptr(cls), alen, 0.0, rc.WEIGHTED, 0.9)
    snap, st = g.snapshot(), g.stats()
    w.hold_rows(snap, sym)
    w.close()
    return snap, st


@pytest.mark.parametrize("alen,heads", [(5, 3), (73, 3), (128, 2)])
def test_heads(amd, alen, heads):
    """rnn_amd_set_multi_step at leakage 0: k_multi_softmax_error.  The infinity is in the stream's own head; the stream's
    other heads are the control's"""
    rows_, where = head_symbols(alen, heads)
    sym = dealt(len(rows_) - len(CLEAN_NAMES))
    ctl = control_of(sym)
    cls = np.array([where[c] if where[c] >= 0 else j % heads for j, c in enumerate(sym)], np.int32)
    own = [rows_[c][h * alen:(h + 1) * alen] for c, h in zip(sym, cls)]
    plain = [rows_[0][h * alen:(h + 1) * alen] for h in cls]
    nxt = np.array([far_target(plain[j]) if j in POISONED else (int(np.argmax(own[j])), far_target(own[j]))[j % 2]
                    for j in range(S)], np.int32)
    assert all(nxt[j] != int(np.argmax(plain[j])) for j in POISONED)
    p, pst = heads_step(amd, alen, heads, sym, nxt, cls, rows_)
    c, cst = heads_step(amd, alen, heads, ctl, nxt, cls, rows_)

    def scored(j):
        m = np.zeros(alen * heads, bool)
        if where[sym[j]] >= 0:
            m[cls[j] * alen:(cls[j] + 1) * alen] = restated_nan(own[j], nxt[j])
            assert m.sum() == alen
        return m

    hold_streams(p, c, sym, scored, alen * heads)
    assert np.array_equal(p["rng"], c["rng"])
    hold_stats(pst, cst, len(POISONED), S)
    assert np.isnan(pst.entropy) and np.isfinite(cst.entropy)


# ------------------------------------------------------------------ class groups --

def group_symbols():
    """-> (rows [symbol][43], (group, size) poisoned per symbol or None, offsets, sizes)"""
    sizes = np.array(le.GROUP_SIZES, np.int32)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int32)
    clean = [np.concatenate([le.rows(int(n), k)[name] for n in sizes]) for k, name in enumerate(CLEAN_NAMES)]
    full, where = list(clean), [None] * len(clean)
    for g, kind in ((4, "pos_inf"), (3, "neg_inf"), (4, "nan"), (3, "both"), (1, "pos_inf")):
        n, o = int(sizes[g]), int(offsets[g])
        r = clean[0].copy()
        row = le.nonfinite_rows(n)[kind]
        r[o:o + n] = np.where(np.isfinite(row), r[o:o + n], row)
        full.append(r)
        where.append(g)
    return full, where, offsets, sizes


def groups_step(amd, one_call, sym, tg, rows_, offsets, sizes):
    nsym, ng = 16, len(sizes)
    w = Written(amd, rows_, nsym, int(sizes.sum()))
    g = w.g
    x = np.zeros((S, nsym), np.float32)
    x[np.arange(S), sym] = 1.0
    trained = np.zeros(S, np.uint8)
    g.stats(clear=True)
    amd.rnn_bptt_clear_deltas(g.net)
    amd.rnn_amd_set_advance(g.handle)
    if one_call:
        amd.rnn_amd_set_opinion_grouped_softmax(g.handle, rc.fptr(x), nsym, ng, rc.iptr(offsets), rc.iptr(sizes), rc.iptr(tg),
                                                None, rc.u8ptr(trained))
    else:
        amd.rnn_amd_set_opinion(g.handle, rc.fptr(x), nsym, None)
        amd.rnn_amd_set_grouped_softmax_error(g.handle, ng, rc.iptr(offsets), rc.iptr(sizes), rc.iptr(tg), None,
                                              rc.u8ptr(trained))
    amd.rnn_amd_set_calc_deltas(g.handle, 1, None, rc.u8ptr(trained))
    snap, st = g.snapshot(), g.stats()
    w.hold_rows(snap, sym)
    w.close()
    return snap, st, trained


@pytest.mark.parametrize("one_call", [False, True])
def test_class_groups(amd, one_call):
    """rnn_amd_set_opinion + rnn_amd_set_grouped_softmax_error (k_grouped_softmax_error) and
    rnn_amd_set_opinion_grouped_softmax (k_text_top<2>): the infinity in ONE group of 30, 7 or 2 outputs; the stream's
    other groups are the control's"""
    rows_, where, offsets, sizes = group_symbols()
    ng, n_out = len(sizes), int(sizes.sum())
    sym = dealt(len(rows_) - len(CLEAN_NAMES))
    ctl = control_of(sym)
    tg = np.zeros((S, ng), np.int32)
    for j in range(S):
        for g in range(ng):
            row = rows_[ctl[j]][offsets[g]:offsets[g] + sizes[g]]
            tg[j, g] = (far_target(row), int(np.argmax(row)), -1)[(j + g) % 3]
        if where[sym[j]] is not None:
            g = where[sym[j]]
            tg[j, g] = far_target(rows_[0][offsets[g]:offsets[g] + sizes[g]])   # trained, and no win in the control
    tg = np.ascontiguousarray(tg)
    p, pst, ptr = groups_step(amd, one_call, sym, tg, rows_, offsets, sizes)
    c, cst, ctr = groups_step(amd, one_call, ctl, tg, rows_, offsets, sizes)

    def scored(j):
        m = np.zeros(n_out, bool)
        g = where[sym[j]]
        if g is not None:
            m[offsets[g]:offsets[g] + sizes[g]] = restated_nan(rows_[sym[j]][offsets[g]:offsets[g] + sizes[g]], tg[j, g])
            assert m.sum() == sizes[g]
        return m

    hold_streams(p, c, sym, scored, n_out)
    assert np.array_equal(ptr, ctr) and ptr.all()
    hold_stats(pst, cst, len(POISONED), int((tg >= 0).sum()))
    assert 0 < cst.correct < cst.count


# ------------------------------------------------------------------ sigmoid --

SIGMOID_N = 3


def sigmoid_symbols():
    """-> rows [symbol][16]: clean rows of sigmoid arguments, then symbol 0's row with outputs that are not finite among
    the first SIGMOID_N (they take the sigmoid) and behind them (they stay as written)"""
    clean = le.sigmoid_case(SIGMOID_N)[:len(CLEAN_NAMES)]
    full = list(clean)
    for entries in (((1, np.inf),), ((0, -np.inf),), ((2, np.nan),), ((0, np.inf), (2, -np.inf), (7, np.inf)),
                    ((9, np.nan), (1, np.nan))):
        r = clean[0].copy()
        for pos, val in entries:
            r[pos] = val
        full.append(r)
    return full


def sigmoid_step(amd, form, sym, tgt, rows_):
    nsym, n, width = 16, SIGMOID_N, le.SIGMOID_WIDTH
    w = Written(amd, rows_, nsym, width)
    g = w.g
    x = np.zeros((S, nsym), np.float32)
    x[np.arange(S), sym] = 1.0
    out = np.full((S, g.O), 7.0, np.float32)
    amd.rnn_bptt_clear_deltas(g.net)
    amd.rnn_amd_set_advance(g.handle)
    if form == "forward only":
        amd.rnn_amd_set_opinion(g.handle, rc.fptr(x), nsym, None)
        amd.rnn_amd_set_sigmoid_outputs(g.handle, n, rc.fptr(out))
    elif form == "one call":
        amd.rnn_amd_set_opinion_sigmoid_mse(g.handle, rc.fptr(x), nsym, rc.fptr(tgt), n, n)
    else:
        amd.rnn_amd_set_opinion(g.handle, rc.fptr(x), nsym, None)
        amd.rnn_amd_set_sigmoid_mse_error(g.handle, rc.fptr(tgt), n, n)
    if form != "forward only":
        amd.rnn_amd_set_calc_deltas(g.handle, 1, None, None)
    snap = g.snapshot()
    snap["fetched"] = out
    for j, c in enumerate(sym):       # behind the first n outputs the row is the written one still: an infinity by its bits
        assert is_written(snap["output"][j, n:width], rows_[c][n:]), j
    w.close()
    return snap


@pytest.mark.parametrize("form", ["two calls", "one call", "forward only"])
def test_sigmoid(amd, form):
    """rnn_amd_set_sigmoid_mse_error (k_sigmoid_mse_error), rnn_amd_set_opinion_sigmoid_mse (k_text_top<1>),
    rnn_amd_set_sigmoid_outputs (k_sigmoid_outputs).  Elementwise: the sigmoid of an output that is not finite is NaN, and
    so is its error; every other output of the same row is the control's"""
    rows_ = sigmoid_symbols()
    n, width = SIGMOID_N, le.SIGMOID_WIDTH
    sym = dealt(len(rows_) - len(CLEAN_NAMES))
    ctl = control_of(sym)
    tgt = np.ascontiguousarray((np.random.default_rng(5).integers(0, 256, (S, n)) / F(255)).astype(np.float32))
    p = sigmoid_step(amd, form, sym, tgt, rows_)
    c = sigmoid_step(amd, form, ctl, tgt, rows_)

    def scored(j):
        m = np.zeros(n, bool)
        m[:] = ~np.isfinite(rows_[sym[j]][:n])
        assert np.array_equal(m, np.isnan(le.fast_sigmoid(rows_[sym[j]][:n])))
        return m

    for j in range(S):
        bad = scored(j)
        assert bad.any() == (j in POISONED)
        keys = ["output"] + (["fetched"] if form == "forward only" else ["o_error"])
        for k in keys:
            assert np.array_equal(np.isnan(p[k][j, :n]), bad), (k, j)
            assert same(p[k][j, :n][~bad], c[k][j, :n][~bad]), (k, j)
            assert np.isfinite(c[k][j, :n]).all()
        if form != "forward only":
            assert same(p["o_error"][j, n:], c["o_error"][j, n:])
        if j in CLEAN:
            assert same(p["hidden"][j], c["hidden"][j]) and same(p["hist"][:, j], c["hist"][:, j])
            assert same(p["output"][j], c["output"][j])


# ------------------------------------------------------------------ cross entropy --

def text_around(bad, length=14, at=5):
    """a text over the clean symbols with symbol `bad` at position `at`"""
    text = np.array([k % len(CLEAN_NAMES) for k in range(length)], np.uint8)
    text[at] = bad
    return text


def test_cross_entropy(amd):
    """rnn_char_cross_entropy: k_xent_accumulate.  A text that feeds a poisoned symbol at a scored step has no cross
    entropy; one that feeds it only before the skip has the control's"""
    n = 42
    names, rows_ = symbols(n)
    got = {}
    for run, rws in (("poisoned", rows_), ("control", twin(rows_))):
        w = Written(amd, rws, n, n, n_streams=1, D=1, batched=False)
        for k in range(len(CLEAN_NAMES), len(rows_)):
            text = text_around(k)
            for skip in (0, 5, 6):
                got[run, k, skip] = amd.rnn_char_cross_entropy(w.g.net, None, rc.u8ptr(text), len(text), skip, None, 0)
        w.close()
    for k in range(len(CLEAN_NAMES), len(rows_)):
        for skip in (0, 5):
            assert np.isnan(got["poisoned", k, skip]) and np.isfinite(got["control", k, skip]), (names[k], skip)
        assert same64(got["poisoned", k, 6], got["control", k, 6]) and np.isfinite(got["control", k, 6]), names[k]


def test_cross_entropy_per_head(amd):
    """rnn_char_multi_cross_entropy: k_multi_xent_accumulate, 3 heads of 73.  The head with the infinity has no cross
    entropy, the others have the control's"""
    alen, heads = 73, 3
    rows_, where = head_symbols(alen, heads)
    got = {}
    for run, rws in (("poisoned", rows_), ("control", twin(rows_))):
        w = Written(amd, rws, alen, alen * heads, n_streams=1, D=1, hidden_size=96, batched=False)
        for k in range(len(CLEAN_NAMES), len(rows_)):
            text = text_around(k)
            for skip in (3, 6):
                ent = (C.c_double * heads)(*([7.0] * heads))
                amd.rnn_char_multi_cross_entropy(w.g.net, rc.u8ptr(text), len(text), alen, ent, skip)
                got[run, k, skip] = np.array(list(ent))
        w.close()
    for k in range(len(CLEAN_NAMES), len(rows_)):
        p, c = got["poisoned", k, 3], got["control", k, 3]
        assert np.isfinite(c).all()
        assert np.array_equal(np.isnan(p), np.arange(heads) == where[k]), (k, p)
        assert same64(p[~np.isnan(p)], c[~np.isnan(p)])
        assert same64(got["poisoned", k, 6], got["control", k, 6])


# ------------------------------------------------------------------ the batched forward-only calls --
# The designed net has no recurrence: a step's output row depends on that step's symbol alone.

class Net:
    """a fresh net without a training set, the written weights in it"""

    def __init__(self, lib, rows_, input_size, output_size, hidden_size=HIDDEN):
        self.lib = lib
        self.net = net = lib.rnn_new(input_size, hidden_size, output_size, rc.FLAG_STANDARD, 1, None, 4, 1e-3, 0.9, 0.0, rc.RELU)
        n = net.contents
        self.I, self.H, self.O = n.i_size, n.h_size, n.o_size
        ih, ho = le.designed_nonfinite_weights(self.I, self.H, self.O, hidden_size, rows_)
        write_weights(lib, net, self.I, self.H, self.O, ih, ho, momentum=False)

    def close(self):
        self.lib.rnn_delete_net(self.net)


def batch_of_texts(n_bad, first=len(CLEAN_NAMES), length=9):
    """twelve texts over the clean symbols and their skips; text j of POISONED holds a poisoned symbol: scored in the middle
    (1, 6), at the first scored step (4: at its skip), only in front of the skip (9: the text is clean all the same), only
    as the last symbol, which is a target and is never fed (11: clean too).  -> (texts, skips, the texts with NaN sums)"""
    texts = [np.array([(j + k) % first for k in range(length + j % 3)], np.uint8) for j in range(S)]
    skips = np.array([j % 3 for j in range(S)], np.int32)
    bad = [first + k % n_bad for k in range(len(POISONED))]
    texts[1][4] = bad[0]
    texts[4][skips[4]] = bad[1]
    texts[6][len(texts[6]) - 2] = bad[2]          # the last symbol that is fed
    skips[9] = 4
    texts[9][3] = bad[3]
    texts[11][len(texts[11]) - 1] = bad[4]
    return texts, skips, (1, 4, 6)


def cleaned(texts, first=len(CLEAN_NAMES)):
    return [np.where(t >= first, 0, t).astype(np.uint8) for t in texts]


def run_texts_raw(lib, net, texts, skips, alphabet_len=0):
    keep, ptrs, lens = text_pointers(texts)
    heads = net.contents.output_size // alphabet_len if alphabet_len else 1
    sums = np.full((len(keep), heads), 7.0)
    out = sums.ctypes.data_as(C.POINTER(C.c_double))
    if alphabet_len:
        r = lib.rnn_amd_run_texts_heads(net, ptrs, rc.iptr(lens), rc.iptr(skips), len(keep), alphabet_len, out)
    else:
        r = lib.rnn_amd_run_texts(net, ptrs, rc.iptr(lens), rc.iptr(skips), len(keep), out)
    assert r == 0
    return sums


@pytest.mark.parametrize("n", [42, 130])
def test_run_texts(amd, n):
    """rnn_amd_run_texts: k_texts_step's scoring half.  A text that feeds a poisoned symbol from its skip on has a NaN sum;
    one that holds it only in front of the skip or as its last symbol, and every clean text, has the control's"""
    names, rows_ = symbols(n)
    texts, skips, nan_texts = batch_of_texts(len(rows_) - len(CLEAN_NAMES))
    got = {}
    for run, rws in (("poisoned", rows_), ("control", twin(rows_))):
        net = Net(amd, rws, n, n)
        got[run] = run_texts_raw(amd, net.net, texts, skips)[:, 0]
        net.close()
    assert np.isfinite(got["control"]).all()
    assert np.array_equal(np.nonzero(np.isnan(got["poisoned"]))[0], nan_texts), got["poisoned"]
    fine = ~np.isnan(got["poisoned"])
    assert same64(got["poisoned"][fine], got["control"][fine])


def test_run_texts_heads(amd):
    """rnn_amd_run_texts_heads, 3 heads of 73: only the head that holds the infinity has a NaN sum"""
    alen, heads = 73, 3
    rows_, where = head_symbols(alen, heads)
    texts, skips, nan_texts = batch_of_texts(len(rows_) - len(CLEAN_NAMES))
    got = {}
    for run, rws in (("poisoned", rows_), ("control", twin(rows_))):
        net = Net(amd, rws, alen, alen * heads, hidden_size=96)
        got[run] = run_texts_raw(amd, net.net, texts, skips, alen)
        net.close()
    want_nan = np.zeros((S, heads), bool)
    for j in nan_texts:
        for c in texts[j]:
            if where[c] >= 0:
                want_nan[j, where[c]] = True
    assert want_nan.sum() == len(nan_texts) and np.isfinite(got["control"]).all()
    assert np.array_equal(np.isnan(got["poisoned"]), want_nan)
    assert same64(got["poisoned"][~want_nan], got["control"][~want_nan])


def trace_raw(lib, net, texts, guard=4):
    keep, ptrs, lens = text_pointers(texts)
    n = len(keep)
    lp = [np.full(len(t) - 1 + guard, 7.0, np.float32) for t in keep]
    gs = [np.full(len(t) - 1 + guard, 0xEE, np.uint8) for t in keep]
    lpp = (rc.c_float_p * n)(*[rc.fptr(a) for a in lp])
    gsp = (rc.c_u8_p * n)(*[rc.u8ptr(a) for a in gs])
    assert lib.rnn_amd_trace_texts(net, ptrs, rc.iptr(lens), n, 0, lpp, gsp) == 0
    for a, b, t in zip(lp, gs, keep):
        assert (a[len(t) - 1:] == 7.0).all() and (b[len(t) - 1:] == 0xEE).all(), "written behind a text's trace"
    return [a[:len(t) - 1] for a, t in zip(lp, keep)], [b[:len(t) - 1] for b, t in zip(gs, keep)]


@pytest.mark.parametrize("n", [42, 130])
def test_trace_texts(amd, n):
    """rnn_amd_trace_texts: texts that are clean, poisoned, clean.  The trace is NaN at exactly the steps that feed a
    poisoned symbol and the control's elsewhere; the guesses are held at the clean steps"""
    names, rows_ = symbols(n)
    first = len(CLEAN_NAMES)
    texts, _, _ = batch_of_texts(len(rows_) - first)
    for k, j in enumerate(POISONED):                  # and one more poisoned step, next to a clean one, in every such text
        texts[j][1] = first + (k + 1) % (len(rows_) - first)
    got = {}
    for run, rws in (("poisoned", rows_), ("control", twin(rows_))):
        net = Net(amd, rws, n, n)
        got[run] = trace_raw(amd, net.net, texts)
        net.close()
    steps = 0
    for j in range(S):
        fed = texts[j][:-1] >= first
        steps += int(fed.sum())
        lp, gs = got["poisoned"][0][j], got["poisoned"][1][j]
        clp, cgs = got["control"][0][j], got["control"][1][j]
        assert np.isfinite(clp).all()
        assert np.array_equal(np.isnan(lp), fed), (j, lp)
        assert same(lp[~fed], clp[~fed]) and np.array_equal(gs[~fed], cgs[~fed]), j
    assert steps >= 2 * len(POISONED) - 2


def test_classify_texts(amd):
    """rnn_amd_classify_texts: k_classify_step.  Every symbol is fed and scored from the skip on: the sums, the sums of
    squares, the error and the entropy of a text with a poisoned symbol there are NaN, the others the control's"""
    n = 42
    names, rows_ = symbols(n)
    first = len(CLEAN_NAMES)
    texts, skips, _ = batch_of_texts(len(rows_) - first)
    nan_texts = (1, 4, 6, 11)                          # (the last symbol is fed and scored here; 9's lies before its skip)
    classes = [np.array([(3 * k + j) % n for k in range(len(t))], np.uint8) for j, t in enumerate(texts)]
    for j in POISONED:                                 # the class of a poisoned step is not the `plain` row's best guess
        for k in np.nonzero(texts[j] >= first)[0]:
            classes[j][k] = far_target(rows_[0])
    got = {}
    for run, tx in (("poisoned", texts), ("control", cleaned(texts))):
        net = Net(amd, rows_, n, n)
        keep, ptrs, lens = text_pointers(tx)
        ckeep = [np.ascontiguousarray(c) for c in classes]
        cptrs = (rc.c_u8_p * S)(*[rc.u8ptr(c) for c in ckeep])
        sums, sumsqs = np.full((S + 1, n), 7.0), np.full((S + 1, n), 7.0)
        scores = np.full(S + 1, -7, np.dtype([("error", np.float64), ("entropy", np.float64), ("correct", np.int64),
                                              ("count", np.int64)]))
        dp = C.POINTER(C.c_double)
        assert amd.rnn_amd_classify_texts(net.net, ptrs, rc.iptr(lens), rc.iptr(skips), cptrs, S, None, None,
                                          sums.ctypes.data_as(dp), sumsqs.ctypes.data_as(dp),
                                          scores.ctypes.data_as(C.POINTER(rc.ClassScore))) == 0
        assert (sums[S] == 7.0).all() and (sumsqs[S] == 7.0).all() and scores[S]["count"] == -7
        got[run] = (sums[:S], sumsqs[:S], scores[:S])
        net.close()
    (ps, pq, pc), (cs, cq, cc) = got["poisoned"], got["control"]
    assert np.isfinite(cs).all() and np.isfinite(cq).all() and np.isfinite(cc["error"]).all() and np.isfinite(cc["entropy"]).all()
    for j in range(S):
        assert pc["count"][j] == cc["count"][j] == len(texts[j]) - max(int(skips[j]), 0)
        if j in nan_texts:
            assert np.isnan(ps[j]).all() and np.isnan(pq[j]).all() and np.isnan(pc["error"][j]) and np.isnan(pc["entropy"][j])
            assert cc["correct"][j] <= pc["correct"][j] <= cc["correct"][j] + int((texts[j] >= first).sum())
        else:
            assert same64(ps[j], cs[j]) and same64(pq[j], cq[j]) and pc["correct"][j] == cc["correct"][j]
            assert same64(pc["error"][j], cc["error"][j]) and same64(pc["entropy"][j], cc["entropy"][j])


def test_run_sequences_with_class_groups(amd):
    """rnn_amd_run_sequences: k_seqs_step.  Groups of 30 and 7 outputs and 7 columns in no group: the group that holds the
    infinity is NaN, the frame's other group is the control's, and a column in no group is copied raw, the infinity by
    its bits"""
    groups = [(0, 30), (30, 7)]
    n_out, nsym = 44, 16
    first = len(CLEAN_NAMES)
    clean = [np.concatenate([le.rows(30, k)[name], le.rows(7, k)[name], le.rows(7, k + 1)[name]])
             for k, name in enumerate(CLEAN_NAMES)]
    rows_, where = list(clean), [None] * first
    for g, kind in ((0, "pos_inf"), (1, "neg_inf"), (0, "nan"), (1, "both"), (2, "pos_inf")):
        o, n = ((0, 30), (30, 7), (37, 7))[g]
        r, row = clean[0].copy(), le.nonfinite_rows(n)[kind]
        r[o:o + n] = np.where(np.isfinite(row), r[o:o + n], row)
        rows_.append(r)
        where.append(g)
    texts, _, _ = batch_of_texts(len(rows_) - first)
    got = {}
    for run, tx in (("poisoned", texts), ("control", cleaned(texts))):
        net = Net(amd, rows_, nsym, n_out)
        seqs = []
        for t in tx:
            x = np.zeros((len(t), nsym), np.float32)
            x[np.arange(len(t)), t] = 1.0
            seqs.append(x)
        frames = np.array([len(s) for s in seqs], np.int32)
        ans = [np.full(len(s) * n_out + 4, 7.0, np.float32) for s in seqs]
        win = [np.full(len(s) * 2 + 4, 0xEE, np.uint8) for s in seqs]
        inp = (rc.c_float_p * S)(*[rc.fptr(s) for s in seqs])
        ansp = (rc.c_float_p * S)(*[rc.fptr(a) for a in ans])
        winp = (rc.c_u8_p * S)(*[rc.u8ptr(a) for a in win])
        goff, gsize = np.array([g[0] for g in groups], np.int32), np.array([g[1] for g in groups], np.int32)
        assert amd.rnn_amd_run_sequences(net.net, inp, rc.iptr(frames), S, nsym, 2, rc.iptr(goff), rc.iptr(gsize), None, None,
                                         0, ansp, winp) == 0
        for a, b, s in zip(ans, win, seqs):
            assert (a[len(s) * n_out:] == 7.0).all() and (b[len(s) * 2:] == 0xEE).all()
        got[run] = ([a[:len(s) * n_out].reshape(-1, n_out) for a, s in zip(ans, seqs)],
                    [b[:len(s) * 2].reshape(-1, 2) for b, s in zip(win, seqs)])
        net.close()
    seen = set()
    for j in range(S):
        for t, c in enumerate(texts[j]):
            pa, ca = got["poisoned"][0][j][t], got["control"][0][j][t]
            pw, cw = got["poisoned"][1][j][t], got["control"][1][j][t]
            assert np.isfinite(ca).all()
            g = where[c]
            seen.add(g)
            for k, (o, n) in enumerate(groups):
                if g == k:
                    assert np.isnan(pa[o:o + n]).all(), (j, t, k)
                else:
                    assert same(pa[o:o + n], ca[o:o + n]) and pw[k] == cw[k], (j, t, k)
            if g == 2:
                assert is_written(pa[37:44], rows_[c][37:44]) and np.isposinf(pa[37:44]).sum() == 1
            else:
                assert same(pa[37:44], ca[37:44])
            assert same(pa[44:], ca[44:])
    assert seen == {None, 0, 1, 2}


def test_continue_texts_ends_a_row_without_a_total_at_the_attempt_cap(amd):
    """rnn_amd_continue_texts: the sampler guards its exponential itself (sample_rule.h).  One prompt ends on a poisoned
    symbol: the call returns -1, that row is empty with nothing written behind it and its generator has made
    SAMPLE_MAX_ATTEMPTS steps (the oracle's generator, stepped on the CPU); every other row is the control's"""
    n, max_len, row = 42, 6, 4
    first = len(CLEAN_NAMES)
    clean = le.rows(n)
    # symbol 42 of 48 inputs: behind the 42 outputs, so that no row can DRAW the poisoned symbol and feed it
    rows_ = [clean[k] for k in CLEAN_NAMES] + [np.zeros(n, np.float32)] * (n - first) + [le.nonfinite_rows(n)["pos_inf"]]
    prompts = [np.array([(j + k) % first for k in range(2 + j % 3)], np.uint8) for j in range(S)]
    prompts[row][-1] = n
    seeds = np.arange(100, 100 + S, dtype=np.uint64)
    got = {}
    for run, tx in (("poisoned", prompts), ("control", cleaned(prompts))):
        net = Net(amd, rows_, n + 6, n)
        keep, ptrs, plens = text_pointers(tx)
        out = np.full((S, max_len), 0xEE, np.uint8)
        lens = np.full(S, -1, np.int32)
        rng = np.zeros((S, 4), np.uint64)
        r = amd.rnn_amd_continue_texts(net.net, ptrs, rc.iptr(plens), seeds.ctypes.data_as(C.POINTER(C.c_uint64)), S, max_len,
                                       0.0, -1, 0, 0, rc.u8ptr(out), rc.iptr(lens), rng.ctypes.data_as(C.POINTER(rc.RandCtx)))
        got[run] = (r, out, lens, rng)
        net.close()
    (pr, pout, plen, prng), (cr, cout, clen, crng) = got["poisoned"], got["control"]
    assert cr == 0 and (clen == max_len).all()
    assert pr == -1 and plen[row] == 0 and (pout[row] == 0xEE).all()
    orc = rc.load_oracle()
    g = rc.OrcRng()
    orc.orc_init_rand64(C.byref(g), int(seeds[row]))
    for _ in range(SAMPLE_MAX_ATTEMPTS):
        orc.orc_rand64(C.byref(g))
    assert np.array_equal(prng[row], np.array([g.a, g.b, g.c, g.d], np.uint64))
    others = np.arange(S) != row
    assert np.array_equal(pout[others], cout[others]) and np.array_equal(plen[others], clen[others])
    assert np.array_equal(prng[others], crng[others])
