"""Many texts traced symbol by symbol in one batched device run (rnn_amd_trace_texts; recur_amd/csrc/texts_api.c,
texts_plan.h, k_texts_step's trace form in kernels_rows.hip) against the oracle: an OracleSet with one stream per text, the
product net's weights copied in, every stream starting from the product net's hidden row (test_gpu_run_texts.oracle_like), then
per step orc_one_hot_opinion, orc_softmax of each head, orc_capped_log2f of the target's likelihood and
orc_softmax_best_guess.

THE BAR is the project's parity bar, applied to each text's logp array against the oracle's: 1e-4 on the 2-norm and on
the largest element, and element by element |a - b| <= 1e-4 |b| on the elements of at least 1e-2 of the array's largest;
below that floor the bound an element at the floor gets, |a - b| <= 1e-4 * 1e-2 * largest.

THE GUESS is teacher-checked: the oracle's likelihood at the device's guess lies within 1e-4, relative, of the oracle's
largest, and where the oracle's best leads its runner-up by more than that the guess is the oracle's.  On rows that are
written rather than learned (test 3) the guess is the oracle's, exactly.

Against rnn_amd_run_texts(_heads) the trace is held bit for bit: both calls lay out the same plan and the same kernel
code produces the floats, so the sum of logp[k][skip:], added one after another in a double, IS that call's sum."""
import os
import re
import subprocess

import numpy as np
import pytest

import erewhon_case as ec
import loss_edge_cases as le
import recur_ctypes as rc
import scenarios as sc
from recur_amd.drivers import TRACE_GUARD, run_texts, text_pointers, trace_texts
from test_gpu_loss_edges import designed
from test_gpu_run_texts import erewhon, forward_clone, hidden_row, oracle_like, rng_of, slices, trained

pytestmark = pytest.mark.gpu
BAR = 1e-4
FLOOR = 1e-2
_long = {}


@pytest.fixture(scope="module")
def amd():
    lib = rc.bind_char(rc.load_amd())
    assert lib.rnn_amd_device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return lib


def oracle_trace(o, k, t, alen=0):
    """stream k of the oracle fed text t: (logp [len - 1][heads], best guess [len - 1][heads], likelihoods
    [len - 1][heads][alen])"""
    alen = alen or o.output_size
    heads = o.output_size // alen
    n = max(len(t) - 1, 0)
    logp, best = np.zeros((n, heads), np.float32), np.zeros((n, heads), np.int64)
    like = np.zeros((n, heads, alen), np.float32)
    err = np.zeros(alen, np.float32)
    for i in range(n):
        ans = np.ctypeslib.as_array(o.orc.orc_one_hot_opinion(o.z, k, int(t[i]), 0.0), shape=(o.O,))
        target = int(t[i + 1])
        for h in range(heads):
            src = np.ascontiguousarray(ans[h * alen:(h + 1) * alen])
            o.orc.orc_softmax(rc.fptr(like[i, h]), rc.fptr(src), alen)
            logp[i, h] = o.orc.orc_capped_log2f(float(like[i, h, target])) if target < alen else -100.0
            best[i, h] = o.orc.orc_softmax_best_guess(rc.fptr(err), rc.fptr(src), alen)
    return logp, best, like


def oracle_traces(o, texts, alen=0):
    return [oracle_trace(o, k, t, alen) for k, t in enumerate(texts)]


def at_the_bar(got, want, what=""):
    """one text's logp array against the oracle's; returns the three figures"""
    assert got.shape == want.shape and got.dtype == np.float32
    if want.size == 0:
        return 0.0, 0.0, 0.0
    g, w = got.astype(np.float64), want.astype(np.float64)
    largest = np.abs(w).max()
    figures = (rc.rel_err(g, w), rc.max_err(g, w), rc.elem_err(g, w, FLOOR))
    assert all(f <= BAR for f in figures), (what, figures)
    small = np.abs(w) < FLOOR * largest
    assert np.all(np.abs(g - w)[small] <= BAR * FLOOR * largest), (what, np.abs(g - w)[small].max())
    return figures


def all_at_the_bar(got, want, what):
    worst = np.zeros(3)
    for k, ((lp, _), (wlp, _, _)) in enumerate(zip(got, want)):
        worst = np.maximum(worst, at_the_bar(lp, wlp, "%s, text %d" % (what, k)))
    print("%s: %d texts, largest differences: 2-norm %.3g, largest element %.3g, element by element %.3g"
          % (what, len(got), *worst))


def margins(like):
    """per step and head: (the oracle's largest likelihood, how far it leads the runner-up, relative to itself)"""
    top2 = np.sort(like.astype(np.float64), axis=-1)[..., -2:]
    return top2[..., 1], (top2[..., 1] - top2[..., 0]) / top2[..., 1]


def teacher_checked(got, want, what):
    """the guesses of a batch against the oracle's likelihoods; returns (steps that close, steps)"""
    close = steps = differ = 0
    for k, ((_, gs), (_, best, like)) in enumerate(zip(got, want)):
        assert gs.shape == best.shape and gs.dtype == np.uint8
        if not gs.size:
            continue
        top, lead = margins(like)
        mine = np.take_along_axis(like.astype(np.float64), gs.astype(np.int64)[..., None], axis=-1)[..., 0]
        assert np.all(mine >= top * (1.0 - BAR)), (what, k, np.argwhere(mine < top * (1.0 - BAR))[:5])
        clear = lead > BAR
        assert np.array_equal(gs[clear], best[clear]), (what, k, np.argwhere((gs != best) & clear)[:5])
        close += int((~clear).sum())
        differ += int((gs != best).sum())
        steps += gs.size
    print("%s: %d guesses, %d where the oracle's best leads by 1e-4 or less, %d not the oracle's" % (what, steps, close, differ))
    return close, steps


def running_sum(x):
    """x added one after another in a double, as the device adds"""
    return float(np.cumsum(np.asarray(x, np.float64))[-1]) if len(x) else 0.0


# ------------------------------------------------------------------ 1. the trace is the scorer, bit for bit --

RAGGED = [600, 1, 2, 3, 64, 65, 600, 0]


@pytest.mark.parametrize("heads", [1, 3])
def test_the_trace_is_the_scorer_bit_for_bit(amd, heads):
    a = trained(amd) if heads == 1 else trained(amd, hidden=99, symbols=42, text_symbols=14)
    alen = 0 if heads == 1 else 14
    net = forward_clone(amd, a.net)
    texts = slices(zip([30000, 31000, 32000, 33000, 34000, 35000, 36000, 37000], RAGGED), symbols=alen or None)
    got = trace_texts(amd, net, texts, alphabet_len=alen)
    assert [lp.shape for lp, _ in got] == [(max(n - 1, 0), heads) for n in RAGGED]
    for skips in ([0] * 8, [5, 0, 0, 5, 0, 10, 0, 0], [max(n - 2, 0) for n in RAGGED]):
        sums = run_texts(amd, net, texts, skips, alphabet_len=alen).reshape(8, heads)
        for k, (lp, _) in enumerate(got):
            mine = [running_sum(lp[skips[k]:, c]) for c in range(heads)]
            assert mine == list(sums[k]), (skips, k, mine, sums[k])
    assert all(np.all(lp < 0) and np.all(lp > -30) for lp, _ in got)  # a few bits each, far from the cap
    # without guesses the floats are the same
    for (lp, _), (lq, none) in zip(got, trace_texts(amd, net, texts, alphabet_len=alen, guesses=False)):
        assert none is None and np.array_equal(lp, lq)
    amd.rnn_delete_net(net)


# ------------------------------------------------------------------ 2. per symbol against the oracle --

# 3326 steps.  After 600 generations the net guesses the two commonest symbols nearly everywhere and a third at about one
# step in 700: the longer slices lie where the oracle, trained on the CPU, guesses it most often (5, 3, 8 and 14 times,
# leading the runner-up by several per cent)
LONG = [(30000, 3), (31000, 17), (155240, 112), (33500, 400), (276787, 800), (370849, 2000)]


def long_trained(lib):
    """test_gpu_run_texts.trained's net shape after 600 generations instead of 60: after 60 the net is close to uniform and
    guesses one symbol"""
    if "net" not in _long:
        a = sc.AmdBatchedSet(lib, **ec.KW)
        a.load_text(np.ascontiguousarray(erewhon()[:20000]))
        for i in range(600):
            lib.rnn_amd_set_char_step(a.handle, i, rc.WEIGHTED, 0.9)
        _long["net"] = a
    return _long["net"]


def test_per_symbol_against_the_oracle(amd):
    """The conditions asserted first are the oracle's alone.  On the oracle trained on the CPU for 600 generations, with the
    erewhon alphabet and these slices: 0 of 3326 steps with the best within 1e-4 of the runner-up, |logp| 1.37 to 10.3 (the
    floor of the longest text is 0.103), 3 symbols guessed (3113, 182 and 31 times), accuracy 0.208; with the weights the
    device trained, on an MI355X, the same figures.  Measured there: 2-norm 5.6e-7, largest element 2.9e-6, element by
    element 1.3e-5; every guess the oracle's."""
    a = long_trained(amd)
    net = forward_clone(amd, a.net)
    texts = slices(LONG)
    o = oracle_like(amd, a, net, len(texts))
    want = oracle_traces(o, texts)
    o.close()
    # from the oracle alone
    logp = np.concatenate([w[0].ravel() for w in want])
    best = np.concatenate([w[1].ravel() for w in want])
    lead = np.concatenate([margins(w[2])[1].ravel() for w in want])
    target = np.concatenate([t[1:] for t in texts])
    accuracy = float(np.mean(best == target))
    print("oracle: %d steps, %d with the best within 1e-4 of the runner-up, |logp| %.3g .. %.3g, %d symbols guessed, accuracy %.3f"
          % (len(logp), int((lead <= BAR).sum()), np.abs(logp).min(), np.abs(logp).max(), len(np.unique(best)), accuracy))
    assert len(logp) == 3326 and (lead <= BAR).sum() <= 0.01 * len(logp)
    for w in want:
        assert np.all(np.abs(w[0]) >= FLOOR * np.abs(w[0]).max())
    assert len(np.unique(best)) >= 3 and 0.1 <= accuracy <= 0.9
    got = trace_texts(amd, net, texts)
    all_at_the_bar(got, want, "600 generations")
    teacher_checked(got, want, "600 generations")
    amd.rnn_delete_net(net)


# ------------------------------------------------------------------ 3. the tie rule and the cap --

@pytest.mark.parametrize("alen,heads", le.XENT)
def test_ties_and_the_cap_on_written_rows(amd, alen, heads):
    """loss_edge_cases.xent_case on a designed net: the output row of a step is written, so the likelihoods are the loss
    kernels' pieces, which tests/test_gpu_loss_edges.py found bit-equal to the oracle's: the guess is the oracle's exactly.
    (The floats themselves are the device's log2f of those likelihoods: on an MI355X 141 of 299 and 1319 of 2106 are the
    host's to the bit, the rest a last place off; they are held at the bar, the cap exactly.)"""
    full, text, slots, _ = le.xent_case(alen, heads)
    scored = le.xent_scored(slots, text)
    tie_names = {name for _, name, _, _ in scored if name.startswith("tie_")}
    across = [n for n in tie_names if int(n.split("_")[1]) % 64 != int(n.split("_")[2]) % 64]
    capped = sum(le.scored(row, t)["xent"] == np.float32(-100) for _, _, row, t in scored)
    print("%d x %d: %d scored steps, ties %s, %d capped likelihoods" % (alen, heads, len(scored), sorted(tie_names), capped))
    assert across and capped >= 1
    g, o = designed(amd, full, alen, alen * heads, 1, D=1, hidden_size=64 if alen <= 64 else 96, batched=False)
    o.arrays()["hidden"][:] = hidden_row(amd, g.net)[None, :]
    wlp, wbest, wlike = oracle_trace(o, 0, text, alen)
    # the oracle reaches what the catalogue says: ties among its likelihoods, and the cap
    assert (wlp == -100).sum() == capped and ((wlike == wlike.max(axis=-1, keepdims=True)).sum(axis=-1) > 1).any()
    (lp, gs), = trace_texts(amd, g.net, [text], alphabet_len=alen if heads > 1 else 0)
    differ = np.argwhere(gs != wbest)
    assert differ.size == 0, [(int(i), int(h), int(gs[i, h]), int(wbest[i, h]), slots[text[i]][h][0]) for i, h in differ[:8]]
    assert np.array_equal(lp == -100, wlp == -100)
    at_the_bar(lp, wlp, "written rows %d x %d" % (alen, heads))
    print("written rows %d x %d: %d of %d floats bit-equal to the oracle's" % (alen, heads, int((lp == wlp).sum()), lp.size))
    g.close()
    o.close()


# ------------------------------------------------------------------ 4. two waves and every small row count --

def test_two_waves_and_every_small_row_count(amd):
    """300 texts of 0 .. 40 symbols, hidden 39: two waves at the default width, every row count from many down to 1"""
    a = trained(amd, hidden=39)
    net = forward_clone(amd, a.net)
    lens = [k % 41 for k in range(300)]
    texts = slices((30000 + 37 * k, n) for k, n in enumerate(lens))
    o = oracle_like(amd, a, net, 300)
    want = oracle_traces(o, texts)
    o.close()
    got = trace_texts(amd, net, texts)  # (asserts the guards behind every array, and that every traced step was written)
    all_at_the_bar(got, want, "300 texts")
    teacher_checked(got, want, "300 texts")
    # the arrays of texts shorter than 2 symbols are untouched, and nothing is written behind any other's entries
    keep, ptrs, ln = text_pointers(texts)
    lp = [np.full(max(n - 1, 0) + TRACE_GUARD, np.nan, np.float32) for n in lens]
    gs = [np.full(max(n - 1, 0) + TRACE_GUARD, 0xEE, np.uint8) for n in lens]
    lpp = (rc.c_float_p * 300)(*[rc.fptr(x) for x in lp])
    gsp = (rc.c_u8_p * 300)(*[rc.u8ptr(x) for x in gs])
    assert amd.rnn_amd_trace_texts(net, ptrs, rc.iptr(ln), 300, 0, lpp, gsp) == 0
    for k, n in enumerate(lens):
        m = max(n - 1, 0)
        assert np.all(np.isnan(lp[k][m:])) and np.all(gs[k][m:] == 0xEE)
        assert np.array_equal(lp[k][:m], got[k][0][:, 0]) and np.array_equal(gs[k][:m], got[k][1][:, 0])
    amd.rnn_delete_net(net)


# ------------------------------------------------------------------ 5. heads beyond the waves, wide and narrow heads --

def small_texts(w, n, at=30000, seed=3):
    lens = [int(x) for x in np.random.default_rng(seed).integers(2, 8, n)]
    lens[0], lens[-1] = 7, 2
    return [np.ascontiguousarray(w.text[at + 37 * k:at + 37 * k + m]) for k, m in enumerate(lens)]


@pytest.mark.parametrize("name,alen,n", [("B", 73, 64), ("D", 0, 64), ("D", 0, 63), ("A", 0, 8)])
def test_heads_beyond_the_waves_wide_and_narrow_heads(amd, name, alen, n):
    """B: 50 heads of 73 over the kernel's 4 waves, alen 73 > 64 lanes; D: 4 outputs, fewer than the lanes, at 64 rows
    (output=o4) and 63 (output=rows); A: hidden 1024.  The nets are tests/test_gpu_texts_wide.py's, built there."""
    from test_gpu_texts_wide import a_clone, wide
    w = wide(amd, name)
    net = a_clone(amd, w)
    texts = small_texts(w, n)
    o = oracle_like(amd, w, net, n)
    want = oracle_traces(o, texts, alen)
    o.close()
    got = trace_texts(amd, net, texts, alphabet_len=alen)
    what = "%s, %d texts" % (name, n)
    all_at_the_bar(got, want, what)
    teacher_checked(got, want, what)
    amd.rnn_delete_net(net)


# ------------------------------------------------------------------ 6. the net is left alone, the order does not matter --

def test_the_net_is_left_alone_and_the_order_does_not_matter(amd):
    lib = amd
    a = trained(lib)
    net, twin = forward_clone(lib, a.net), forward_clone(lib, a.net)
    prefix = np.ascontiguousarray(erewhon()[29000:29100])
    for x in (net, twin):
        assert lib.rnn_char_prime(x, None, rc.u8ptr(prefix), len(prefix)) == int(prefix[-1])
    hid, rng = hidden_row(lib, net), rng_of(lib, net)
    assert np.array_equal(hid, hidden_row(lib, twin)) and np.any(hid[1:] != 0)
    texts = slices([(30000, 50), (31000, 120), (32000, 33), (33000, 2), (34000, 1), (35000, 120)])
    got = trace_texts(lib, net, texts)
    # hidden row bit for bit, generator, and what the net computes next: a twin that never saw the call
    assert np.array_equal(hidden_row(lib, net), hid) and rng_of(lib, net) == rng
    seg = texts[1]
    mine = lib.rnn_char_cross_entropy(net, None, rc.u8ptr(seg), len(seg), 3, None, 0)
    twins = lib.rnn_char_cross_entropy(twin, None, rc.u8ptr(seg), len(seg), 3, None, 0)
    print("after the trace", mine, "a twin that never saw it", twins)
    assert mine == twins
    # the primed state was the start: the oracle from that hidden row (the twin has moved on; the saved row serves)
    for x in (net, twin):
        lib.rnn_amd_sync_host(x, rc.RNN_AMD_STREAM)
        rc.view(x.contents.hidden_layer, a.H)[:] = hid
        lib.rnn_amd_host_written(x, rc.RNN_AMD_STREAM)
    o = oracle_like(lib, a, net, len(texts))
    all_at_the_bar(got, oracle_traces(o, texts), "primed")
    o.close()
    # a permuted batch gives every text the same arrays bit for bit
    perm = [3, 5, 0, 4, 2, 1]
    again = trace_texts(lib, net, [texts[k] for k in perm])
    for at, k in enumerate(perm):
        assert np.array_equal(again[at][0], got[k][0]) and np.array_equal(again[at][1], got[k][1])
    lib.rnn_delete_net(twin)
    lib.rnn_delete_net(net)


# ------------------------------------------------------------------ 7. the tool --

ESCAPE = re.compile("\033\\[[0-9;]*m")


def test_the_tool_traces_and_colours(amd, tmp_path):
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

    def output(args):
        r = subprocess.run(tool + args + names, capture_output=True, timeout=300, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.decode("utf-8")

    def encode(alphabet, data):
        import ctypes as C
        n = C.c_int(0)
        p = lib.rnn_char_alloc_encoded_text(alphabet, data, len(data), C.byref(n), None, False)
        return np.ctypeslib.as_array(p, shape=(n.value,)).copy()

    net = lib.rnn_load_net(path.encode())
    alphabet = lib.rnn_char_new_alphabet_from_net(net)
    points = [alphabet.contents.points[i] for i in range(alphabet.contents.len)]
    texts = [encode(alphabet, f.read_bytes()) for f in files]
    lib.rnn_char_free_alphabet(alphabet)
    lib.rnn_delete_net(net)
    independent = output(["-I"]).splitlines()
    assert [x.rsplit(" ", 1)[0] for x in independent] == names
    # -t: len - 1 lines per file, then the -I line; the bits from index 6 on add up to it, to the printed digits
    lines = output(["-t"]).splitlines()
    at = 0
    for k, (name, t) in enumerate(zip(names, texts)):
        rows = [x.split(" ") for x in lines[at:at + len(t) - 1]]
        at += len(t) - 1
        assert all(x[0] == name and len(x) == 5 for x in rows)
        assert [int(x[1]) for x in rows] == list(range(1, len(t)))
        assert [int(x[2]) for x in rows] == [points[s] for s in t[1:]]
        assert all(int(x[4]) in points for x in rows)
        bits = np.array([np.float32(x[3]) for x in rows])
        assert np.all(bits > 0) and np.all(bits < 30)
        figure = running_sum(-bits[5:]) / -(len(t) - 5 - 1)
        assert lines[at] == independent[k] == "%s %.5f" % (name, figure), (lines[at], independent[k], figure)
        at += 1
    assert at == len(lines)
    # -c: the text through the alphabet once the escape sequences are gone, in more than one colour
    coloured = output(["-c", "3", "-d", "0.5"])
    assert len(set(ESCAPE.findall(coloured)) - {"\033[0m"}) > 1
    plain = ESCAPE.sub("", coloured)
    want = "".join("".join(chr(points[s]) for s in t) + "\n" + line + "\n" for t, line in zip(texts, independent))
    assert plain == want
    assert plain.splitlines()[-1] == independent[-1]
