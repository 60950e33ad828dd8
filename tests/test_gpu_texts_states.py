"""The batched text calls with a state per text (rnn_amd_run_texts_from, rnn_amd_trace_texts_from,
rnn_amd_continue_texts_from, rnn_amd_char_score_and_continue_texts; recur_amd/csrc/texts_api.c, sample_api.c,
texts_states.h, the null hid0 of the k_texts_* kernels in kernels_rows.hip) on the device.

Three kinds of claim, each with the check it can bear:
  * bit for bit, where two calls run the same launches on the same values: NULL states against the plain calls; the net's
    own row handed in as every text's state (with NaN where a state carries nothing); texts of EQUAL lengths cut at equal
    places -- every pass of either run then has the same row count and gets the same forward form (fwd_plan.h) --, so a
    trace in two chunks, a continuation in two instalments and a prompt scored and then continued are the uncut calls.
  * at the project's parity bar against the oracle, where row counts differ or the reference is another machine: sums by
    test_gpu_run_texts.at_the_bar; hidden rows by `state_bar`, the README's bar for an array -- 1e-4 on the 2-norm, on
    the largest element, and element by element on the elements at least 1e-2 of the largest -- over the elements
    [1, hidden_size] that carry a state.  Oracle streams take per-stream start states through o.arrays()["hidden"][k];
    where a device state is the start of a second call it is written into the oracle's stream first, so that the second
    comparison does not inherit the first one's difference.
  * teacher-forced, where symbols are drawn: test_gpu_continue_texts.checked's conditions, unchanged, on continuations
    that start from handed-in states (`followed`).

Measured on an MI355X (the largest figures this module printed; the bar is 1e-4; profiles/r07_states_rate.txt): hidden
rows against the oracle's 5.4e-7 on the 2-norm, 5.5e-7 on the largest element, 2.6e-5 element by element; sums from
handed-in states 3.4e-7; the final states of ragged chunks and of windows of 128 equal to the uncut call's to the bit.

The nets are test_gpu_run_texts.trained()'s; hidden 1024 is test_gpu_texts_wide's net A."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import recur_ctypes as rc
import sample_oracle as so
from recur_amd.drivers import (continue_texts, continue_texts_from, run_texts, run_texts_from, trace_texts,
                               trace_texts_from)
from test_gpu_continue_texts import (RAGGED, SPACE, char_continue_texts, encoded, primed, prompts_of,
                                     seeds_that_stop_early)
from test_gpu_run_texts import (at_the_bar, erewhon, forward_clone, hidden_row, oracle_like, oracle_sums, rng_of, slices,
                                trained)

pytestmark = pytest.mark.gpu
BAR = 1e-4
LENS = [600, 1, 2, 3, 64, 65, 600, 0]


@pytest.fixture(scope="module")
def amd():
    lib = rc.bind_char(rc.load_amd())
    assert lib.rnn_amd_device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return lib


def carried(states, hidden):
    """the elements of states that carry one"""
    return np.asarray(states)[..., 1:hidden + 1]


def state_bar(got, want, hidden, what):
    """every row of got against the same row of want at the README's bar for an array"""
    got, want = carried(got, hidden), carried(want, hidden)
    assert got.shape == want.shape and got.ndim == 2
    worst = np.zeros(3)
    for g, w in zip(got, want):
        worst = np.maximum(worst, [rc.rel_err(g, w), rc.max_err(g, w), rc.elem_err(g, w)])
    print("%s: %d hidden rows, largest difference 2-norm %.3g, largest element %.3g, element by element %.3g"
          % (what, len(got), *worst))
    assert np.all(worst <= BAR), (what, worst)


def same_traces(one, two):
    return len(one) == len(two) and all(np.array_equal(a, c) and np.array_equal(b, d) for (a, b), (c, d) in zip(one, two))


def same_texts(one, two):
    return len(one) == len(two) and all(np.array_equal(x, y) for x, y in zip(one, two))


def dirty(states, hidden):
    """NaN wherever a state carries nothing: element 0 and the padding"""
    out = np.array(states, np.float32)
    out[:, 0] = np.nan
    out[:, hidden + 1:] = np.nan
    return out


def device_states(lib, a, net, n, at=20000, what="prefixes"):
    """n distinct states from the device itself -- the states behind n different 50-symbol prefixes --, held to oracle
    streams fed the same prefixes"""
    prefixes = slices((at + 211 * k, 50) for k in range(n))
    none, states = run_texts_from(lib, net, prefixes, sums=False)
    assert none is None
    o = oracle_like(lib, a, net, n)
    for k, p in enumerate(prefixes):
        primed(o, k, p, a.output_size)
    state_bar(states, o.arrays()["hidden"], a.hidden_size, what)
    o.close()
    assert len({carried(s, a.hidden_size).tobytes() for s in states}) == n
    return states


def oracle_from(lib, a, net, states):
    """one oracle stream per state, starting from it"""
    o = oracle_like(lib, a, net, len(states))
    o.arrays()["hidden"][:, 1:a.hidden_size + 1] = carried(states, a.hidden_size)
    return o


def sums_and_states(o, a, texts, skips):
    """oracle_sums, and every stream fed its text but the last symbol also where nothing of it is scored (oracle_sums does
    not ask the oracle then), so that the streams' hidden rows are the states the texts end in"""
    want = oracle_sums(o, texts, skips)
    for k, (t, skip) in enumerate(zip(texts, skips)):
        if len(t) >= 2 and not len(t) - 1 > skip:
            primed(o, k, t, a.output_size)
    return want


def followed(o, a, prompts, seeds, texts, rngs, max_len, bias, stop=-1, what=""):
    """test_gpu_continue_texts.checked's conditions on continuations the caller has made: oracle stream k, wherever it
    stands, follows the device's text k from prompts[k][-1] with a generator seeded seeds[k]"""
    alen = a.output_size
    steps = differing = close = exact_rows = 0
    for k, t in enumerate(texts):
        assert 1 <= len(t) <= max_len and np.all(t < alen)
        assert (len(t) == max_len or t[-1] == stop) and not np.any(t[:-1] == stop)
        r = so.replay(o, k, prompts[k][-1], seeds[k], t, bias, alen, 0)
        steps += len(t)
        differing += r.differing(t)
        close += len(r.close)
        if not r.close:
            exact_rows += 1
            assert list(t) == r.strict, (k, list(t), r.strict)
            assert tuple(int(x) for x in rngs[k]) == r.rng, k
        if bias >= so.GREEDY_BIAS:
            assert tuple(int(x) for x in rngs[k]) == so.words(so.seeded(o.orc, seeds[k]))  # no draw: untouched
    print("%s: %d prompts, %d steps, %d picks differ from the oracle's strict pick, %d steps within %g of a boundary (%.2f %%), "
          "%d texts compared exactly" % (what, len(texts), steps, differing, close, so.TOL, 100.0 * close / steps, exact_rows))
    assert steps >= 300  # (of the test's design, not of the library: the 5 % below is not a matter of luck)
    assert differing <= max(1, 0.002 * steps)
    assert close < 0.05 * steps


# ---- 1, 2: NULL states, and the net's own row as every state


def plain_and_from(lib, net, texts, skips, prompts, seeds, states=None, hidden=None):
    """the three plain calls and their _from forms on the same batch: all of it bit for bit"""
    kw = {} if states is None else {"h_in": states}
    sums, _ = run_texts_from(lib, net, texts, skips, want_out=states is not None, **kw)
    assert np.array_equal(sums, run_texts(lib, net, texts, skips))
    assert sums[0] < -100 and sums[1] == 0.0
    traced, _ = trace_texts_from(lib, net, texts, want_out=states is not None, **kw)
    assert same_traces(traced, trace_texts(lib, net, texts))
    for bias in (0.0, 200.0):
        got, rngs, _ = continue_texts_from(lib, net, prompts, seeds, 40, bias, want_out=states is not None, **kw)
        want, wrngs = continue_texts(lib, net, prompts, seeds, 40, bias)
        assert same_texts(got, want) and np.array_equal(rngs, wrngs)
    got, rngs, _ = continue_texts_from(lib, net, prompts, seeds, 40, 0.0, stop=SPACE, want_out=states is not None, **kw)
    want, wrngs = continue_texts(lib, net, prompts, seeds, 40, 0.0, stop=SPACE)
    assert same_texts(got, want) and np.array_equal(rngs, wrngs)


def test_null_states_are_the_plain_calls_bit_for_bit(amd):
    a = trained(amd)
    net = forward_clone(amd, a.net)
    prefix = np.ascontiguousarray(erewhon()[29000:29100])   # (a hidden row that is not zeros)
    amd.rnn_char_prime(net, None, rc.u8ptr(prefix), len(prefix))
    texts = slices(zip([30000, 31000, 32000, 33000, 34000, 35000, 36000, 37000], LENS))
    plain_and_from(amd, net, texts, [5, 0, 0, 5, 0, 10, 0, 0], prompts_of(RAGGED), [100 + k for k in range(8)])
    # heads: [n_texts][n_heads]
    sums, _ = run_texts_from(amd, net, texts, alphabet_len=14, want_out=False)
    assert sums.shape == (8, 3) and np.array_equal(sums, run_texts(amd, net, texts, alphabet_len=14))
    amd.rnn_delete_net(net)


@pytest.mark.parametrize("hidden,symbols", [(130, 73), (39, 42)])
def test_the_nets_own_row_as_every_start_is_the_plain_call_and_nans_are_harmless(amd, hidden, symbols):
    """h_size 132 for hidden 130: one padding float; 40 for hidden 39: none"""
    a = trained(amd, hidden=hidden, symbols=symbols)
    net = forward_clone(amd, a.net)
    prefix = np.ascontiguousarray(erewhon(symbols)[29000:29100])
    amd.rnn_char_prime(net, None, rc.u8ptr(prefix), len(prefix))
    row = hidden_row(amd, net)
    assert a.H == {130: 132, 39: 40}[hidden] and np.abs(row[1:hidden + 1]).max() > 0.01   # with and without padding
    states = dirty(np.tile(row, (8, 1)), hidden)
    assert np.isnan(states[:, 0]).all() and np.isnan(states[:, hidden + 1:]).all() and not np.isnan(carried(states, hidden)).any()
    texts = slices(zip([30000, 31000, 32000, 33000, 34000, 35000, 36000, 37000], LENS), symbols)
    plain_and_from(amd, net, texts, [5, 0, 0, 5, 0, 10, 0, 0], prompts_of(RAGGED, symbols), [100 + k for k in range(8)],
                   states=states, hidden=hidden)
    # and what comes back carries no NaN where a state carries one
    _, back = run_texts_from(amd, net, texts, h_in=states)
    assert not np.isnan(carried(back, hidden)).any()
    assert np.array_equal(carried(back[[1, 7]], hidden), carried(states[[1, 7]], hidden))   # texts without a forward pass
    amd.rnn_delete_net(net)


# ---- 3: distinct starts against the oracle


def test_distinct_starts_against_the_oracle(amd):
    lib = amd
    a = trained(lib)
    net = forward_clone(lib, a.net)
    states = device_states(lib, a, net, 8)
    lens = [64, 1, 200, 3, 65, 2, 130, 0]            # a caller's order that is not the plan's
    skips = [5, 0, 10, 0, 0, 0, 3, 0]
    texts = slices(zip([30000 + 1000 * k for k in range(8)], lens))
    o = oracle_from(lib, a, net, states)
    want = sums_and_states(o, a, texts, skips)
    kept = states.copy()
    got, back = run_texts_from(lib, net, texts, skips, h_in=states)
    assert np.array_equal(states, kept)
    at_the_bar(got, want, "from 8 states")
    short = [k for k, n in enumerate(lens) if n <= 65]
    state_bar(back[short], o.arrays()["hidden"][short], a.hidden_size, "h_out after up to 64 steps from 8 states")
    # the states matter: from the net's own row the figures are others
    assert np.all(np.abs(run_texts(lib, net, texts, skips)[want != 0] - got[want != 0]) > 1e-6)
    # the trace's floats, added up in a double, are those sums, and its states those states, bit for bit
    traced, tback = trace_texts_from(lib, net, texts, h_in=states)
    sums = [float(np.sum(lp[s:, 0].astype(np.float64))) if len(lp) > s else 0.0 for (lp, _), s in zip(traced, skips)]
    at_the_bar(sums, want, "traced from 8 states")
    assert np.array_equal(carried(tback, a.hidden_size), carried(back, a.hidden_size))
    o.close()
    lib.rnn_delete_net(net)


def test_two_waves_of_states_and_every_small_row_count(amd):
    """300 texts of 0 .. 40 symbols from 300 states: two waves, the states of the second behind the first's"""
    lib = amd
    a = trained(lib, hidden=39)
    net = forward_clone(lib, a.net)
    eight = device_states(lib, a, net, 8, what="hidden 39 prefixes")
    states = np.ascontiguousarray(eight[[(3 * k) % 8 for k in range(300)]])
    lens = [k % 41 for k in range(300)]
    skips = [int(x) for x in np.random.default_rng(11).integers(0, 8, 300)]
    texts = slices((30000 + 37 * k, n) for k, n in enumerate(lens))
    o = oracle_from(lib, a, net, states)
    want = sums_and_states(o, a, texts, skips)
    got, back = run_texts_from(lib, net, texts, skips, h_in=states)
    at_the_bar(got, want, "300 texts from 300 states")
    state_bar(back, o.arrays()["hidden"], a.hidden_size, "h_out of 300 texts")
    o.close()
    lib.rnn_delete_net(net)


# ---- 4, 5: chunks


def chunked_trace(lib, net, texts, cut, hidden):
    whole, end = trace_texts_from(lib, net, texts)
    one, mid = trace_texts_from(lib, net, [t[:cut + 1] for t in texts])
    two, last = trace_texts_from(lib, net, [t[cut:] for t in texts], h_in=mid)
    for (lp, gs), (lp1, gs1), (lp2, gs2) in zip(whole, one, two):
        assert len(lp1) == cut and len(lp1) + len(lp2) == len(lp)
        assert np.array_equal(np.concatenate([lp1, lp2]), lp) and np.array_equal(np.concatenate([gs1, gs2]), gs)
    assert np.array_equal(carried(last, hidden), carried(end, hidden))
    assert not np.array_equal(carried(mid, hidden), carried(end, hidden))
    return whole


@pytest.mark.parametrize("hidden,symbols", [(99, 42), (130, 73)])
def test_a_trace_in_two_chunks_is_the_whole_trace_bit_for_bit(amd, hidden, symbols):
    a = trained(amd, hidden=hidden, symbols=symbols)
    net = forward_clone(amd, a.net)
    texts = slices(((30000 + 500 * k, 97) for k in range(8)), symbols)
    whole = chunked_trace(amd, net, texts, 40, hidden)
    assert all(-100.0 < lp.min() and lp.max() <= 0.0 for lp, _ in whole)
    amd.rnn_delete_net(net)


def test_a_trace_in_two_chunks_at_hidden_1024(amd):
    from test_gpu_texts_wide import a_clone, wide
    w = wide(amd, "A")
    net = a_clone(amd, w)
    texts = [np.ascontiguousarray(w.text[30000 + 41 * k:30000 + 41 * k + 33]) for k in range(64)]
    chunked_trace(amd, net, texts, 16, 1024)
    amd.rnn_delete_net(net)


def test_ragged_chunks_at_the_bar(amd):
    """ragged lengths and ragged cut points, a cut at a text's first and at its last symbol among them: the parts' sums
    added against the oracle's whole sums"""
    lib = amd
    a = trained(lib)
    net = forward_clone(lib, a.net)
    lens = [200, 64, 2, 130, 65, 9, 33, 77]
    cuts = [128, 0, 1, 129, 17, 4, 32, 50]
    texts = slices(zip([30000 + 1000 * k for k in range(8)], lens))
    o = oracle_like(lib, a, net, 8)
    want = oracle_sums(o, texts, [0] * 8)
    one, mid = run_texts_from(lib, net, [t[:c + 1] for t, c in zip(texts, cuts)])
    two, end = run_texts_from(lib, net, [t[c:] for t, c in zip(texts, cuts)], h_in=mid)
    assert one[1] == 0.0 and two[3] == 0.0
    at_the_bar(one + two, want, "two ragged chunks")
    whole, wend = run_texts_from(lib, net, texts)
    state_bar(end, wend, a.hidden_size, "the chunks' final states against the uncut call's")
    # windows of 128 symbols, states in place: the rows that have ended feed nothing and keep their state
    states = np.tile(hidden_row(lib, net), (8, 1))
    total = np.zeros(8)
    for at in range(0, max(lens) - 1, 127):
        part, _ = run_texts_from(lib, net, [t[at:at + 128] for t in texts], h_in=states, in_place=True)
        total += part
    at_the_bar(total, want, "windows of 128")
    state_bar(states, wend, a.hidden_size, "the windows' final states against the uncut call's")
    o.close()
    lib.rnn_delete_net(net)


# ---- 6, 7, 8: continuations


@pytest.mark.parametrize("bias", [0.0, 1.0, 200.0])
def test_a_continuation_in_instalments_is_the_continuation(amd, bias):
    a = trained(amd)
    net = forward_clone(amd, a.net)
    prompts = prompts_of([17] * 8)
    seeds = [100 + k for k in range(8)]
    whole, wrngs, wend = continue_texts_from(amd, net, prompts, seeds, 40, bias)
    one, rngs, mid = continue_texts_from(amd, net, prompts, seeds, 15, bias)
    assert all(len(t) == 15 for t in one)
    two, rngs2, end = continue_texts_from(amd, net, [t[-1:] for t in one], None, 25, bias, h_in=mid, rng_in=rngs)
    assert same_texts([np.concatenate(p) for p in zip(one, two)], whole)
    assert np.array_equal(rngs2, wrngs) and np.array_equal(carried(end, a.hidden_size), carried(wend, a.hidden_size))
    seeded = np.array([so.words(so.seeded(rc.load_oracle(), s)) for s in seeds], np.uint64)
    assert np.array_equal(wrngs, seeded) == (bias >= so.GREEDY_BIAS)    # greedy: the generators are untouched
    assert len({t.tobytes() for t in whole}) == 8
    amd.rnn_delete_net(net)


def test_score_then_continue_feeds_a_prompt_once(amd):
    lib = amd
    a = trained(lib)
    net = forward_clone(lib, a.net)
    seeds = [100 + k for k in range(8)]
    # equal lengths: the composition is the one call, bit for bit
    prompts = prompts_of([17] * 8)
    sums, states = run_texts_from(lib, net, prompts)
    assert np.array_equal(sums, run_texts(lib, net, prompts))
    got, rngs, _ = continue_texts_from(lib, net, [p[-1:] for p in prompts], seeds, 40, h_in=states)
    want, wrngs = continue_texts(lib, net, prompts, seeds, 40)
    assert same_texts(got, want) and np.array_equal(rngs, wrngs)
    # ragged: teacher-forced by the oracle, which is fed each prompt but its last symbol
    prompts = prompts_of(RAGGED)
    sums, states = run_texts_from(lib, net, prompts)
    assert np.array_equal(sums, run_texts(lib, net, prompts))
    for bias in (0.0, 1.0):
        texts, rngs, _ = continue_texts_from(lib, net, [p[-1:] for p in prompts], seeds, 40, bias, h_in=states)
        o = oracle_like(lib, a, net, 8)
        for k, p in enumerate(prompts):
            primed(o, k, p, a.output_size)
        followed(o, a, prompts, seeds, texts, rngs, 40, bias, what="scored, then continued, bias %g" % bias)
        o.close()
    lib.rnn_delete_net(net)


def test_stopped_rows_hand_back_the_state_before_the_stop_symbol(amd):
    lib = amd
    a = trained(lib)
    net = forward_clone(lib, a.net)
    n, max_len = 16, 30
    prompts = prompts_of([1 + (7 * k) % 23 for k in range(n)], apart=41)
    seeds = seeds_that_stop_early(lib, a, net, prompts[:4], 20) + [900 + k for k in range(4, n)]
    texts, rngs, states = continue_texts_from(lib, net, prompts, seeds, max_len, 0.0, stop=SPACE)
    assert all(len(t) <= 20 and t[-1] == SPACE for t in texts[:4])
    # the oracle after the prompt and out[k][:-1]: the last symbol written is never fed
    o = oracle_like(lib, a, net, n)
    for k, p in enumerate(prompts):
        primed(o, k, p, a.output_size)
        so.replay(o, k, p[-1], seeds[k], texts[k], 0.0, a.output_size, 0)
    state_bar(states, o.arrays()["hidden"], a.hidden_size, "h_out of rows that stopped and rows that ran out")
    # resumed from the last symbol -- the space, for a stopped row --, teacher-forced from the device's states
    assert all(t[-1] == SPACE for t in texts[:4])
    o.arrays()["hidden"][:, 1:a.hidden_size + 1] = carried(states, a.hidden_size)
    again = [2000 + k for k in range(n)]
    last = [t[-1:] for t in texts]
    more, mrngs, _ = continue_texts_from(lib, net, last, again, 40, 0.0, h_in=states)
    followed(o, a, last, again, more, mrngs, 40, 0.0, what="resumed behind the last symbol")
    o.close()
    lib.rnn_delete_net(net)


# ---- 9: in place, and the net left alone


@pytest.mark.parametrize("kind", ["training", "forward"])
def test_in_place_and_the_net_left_alone(amd, kind):
    lib = amd
    a = trained(lib)
    if kind == "training":
        net, twin = a.nets[2], a.nets[3]
    else:
        net, twin = forward_clone(lib, a.net), forward_clone(lib, a.net)
    lib.rnn_amd_sync_host(twin, rc.RNN_AMD_STREAM)
    rc.view(twin.contents.hidden_layer, a.H)[:] = hidden_row(lib, net)
    lib.rnn_amd_host_written(twin, rc.RNN_AMD_STREAM)
    prefix = np.ascontiguousarray(erewhon()[29000:29100])
    for x in (net, twin):
        assert lib.rnn_char_prime(x, None, rc.u8ptr(prefix), len(prefix)) == int(prefix[-1])
    hid, rng = hidden_row(lib, net), rng_of(lib, net)
    states = device_states(lib, a, net, 8, what="prefixes (" + kind + ")")
    kept = states.copy()
    texts = slices(zip([30000 + 1000 * k for k in range(8)], [50, 1, 120, 33, 2, 0, 65, 64]))
    prompts = prompts_of(RAGGED)
    seeds = [60 + k for k in range(8)]
    hs = a.hidden_size
    # apart
    sums, out = run_texts_from(lib, net, texts, h_in=states)
    traced, tout = trace_texts_from(lib, net, texts, h_in=states)
    conts, crngs, cout = continue_texts_from(lib, net, prompts, seeds, 20, h_in=states)
    assert np.array_equal(states, kept)              # the caller's h_in is read, not written
    # in place
    for call, want in ((lambda s: run_texts_from(lib, net, texts, h_in=s, in_place=True), (sums, out)),
                       (lambda s: trace_texts_from(lib, net, texts, h_in=s, in_place=True), (traced, tout)),
                       (lambda s: continue_texts_from(lib, net, prompts, seeds, 20, h_in=s, in_place=True), (conts, crngs, cout))):
        mine = kept.copy()
        got = call(mine)
        assert got[-1] is not None and np.shares_memory(got[-1], mine)
        assert np.array_equal(carried(mine, hs), carried(want[-1], hs))
        if len(want) == 3:
            assert same_texts(got[0], want[0]) and np.array_equal(got[1], want[1])
        elif isinstance(want[0], list):
            assert same_traces(got[0], want[0])
        else:
            assert np.array_equal(got[0], want[0])
    assert not np.array_equal(carried(out, hs), carried(kept, hs))
    # the net is where it was: hidden row bit for bit, generator, and what it computes next
    assert np.array_equal(hidden_row(lib, net), hid) and rng_of(lib, net) == rng
    seg = texts[2]
    mine = lib.rnn_char_cross_entropy(net, None, rc.u8ptr(seg), len(seg), 3, None, 0)
    twins = lib.rnn_char_cross_entropy(twin, None, rc.u8ptr(seg), len(seg), 3, None, 0)
    print("after the calls", mine, "a twin that never saw them", twins)
    assert mine == twins
    # h_in NULL and h_out wanted: a text without a forward pass gets the net's row as it now stands -- after a priming on
    # the device, which leaves the host's copy behind -- read and not moved
    assert lib.rnn_char_prime(net, None, rc.u8ptr(prefix[:40]), 40) == int(prefix[39])
    _, back = run_texts_from(lib, net, texts)
    now = hidden_row(lib, net)
    assert np.array_equal(carried(back[[1, 5]], hs), np.tile(now[1:hs + 1], (2, 1))) and not np.array_equal(now, hid)
    if kind == "forward":
        lib.rnn_delete_net(twin)
        lib.rnn_delete_net(net)


# ---- 10: the character layer and the tool


def score_and_continue(lib, net, alphabet, prompts, seeds, repeats, char_len, bias, stop, byte_len):
    n, rows = len(prompts), len(prompts) * repeats
    assert len(seeds) == rows
    bufs = [C.create_string_buffer(max(byte_len, 1)) for _ in range(rows)]
    dest = (C.c_char_p * rows)(*[C.cast(b, C.c_char_p) for b in bufs])
    ps = (C.c_char_p * n)(*prompts)
    pb = np.array([len(p) for p in prompts], np.int32)
    sd = np.ascontiguousarray(seeds, np.uint64)
    nbytes = np.full(rows, -1, np.int32)
    entropy = np.full(n, np.nan)
    r = lib.rnn_amd_char_score_and_continue_texts(net, alphabet, ps, rc.iptr(pb), sd.ctypes.data_as(C.POINTER(C.c_uint64)), n,
                                                  repeats, char_len, bias, stop, dest, byte_len, rc.iptr(nbytes),
                                                  entropy.ctypes.data_as(C.POINTER(C.c_double)))
    return r, [b.value for b in bufs], list(nbytes), entropy


def launches(lib):
    """the library's launch counts by class since the last reset (rnn_amd_kernel_time_ms), then reset"""
    counts = []
    for which in range(5):
        n = C.c_long(0)
        lib.rnn_amd_kernel_time_ms(which, C.byref(n), 0)
        counts.append(n.value)
    lib.rnn_amd_kernel_time_ms(0, None, 1)
    return counts


def test_the_char_layer_scores_and_continues_feeding_each_prompt_once(amd):
    lib = amd
    a = trained(lib)
    net = forward_clone(lib, a.net)
    alphabet = rc.default_text_alphabet(lib)
    raw = [b"The  higher Alps", b"and  WHAT then?", b"a", b"of the mountain"]
    prompts = [encoded(lib, alphabet, p) for p in raw]
    assert [len(p) for p in prompts] == [15, 14, 1, 15]
    seeds = [21 + i for i in range(12)]
    r, texts, nbytes, entropy = score_and_continue(lib, net, alphabet, raw, seeds[:4], 1, 40, 0.0, -1, 400)
    assert r == 0 and nbytes == [40] * 4
    # the figures are rnn_amd_char_cross_entropy_texts's, bit for bit (a one-symbol prompt: that call's 0 / -0)
    keep = [np.ascontiguousarray(p) for p in prompts]
    ptrs = (rc.c_u8_p * 4)(*[rc.u8ptr(p) for p in keep])
    want = np.full(4, 123.0)
    assert lib.rnn_amd_char_cross_entropy_texts(net, alphabet, ptrs, rc.iptr(np.array([len(p) for p in keep], np.int32)), 4, 0,
                                                None, 0, want.ctypes.data_as(C.POINTER(C.c_double))) == 0
    print("bits per symbol", entropy, want)
    assert np.array_equal(entropy, want, equal_nan=True) and 1.0 < entropy[0] < 8.0 and np.isnan(entropy[2])
    # prompts that encode to equal lengths, once each: rnn_amd_char_continue_texts's passages
    equal = [raw[0], raw[3], b"it was a long w", b"erewhon or over"]
    assert [len(encoded(lib, alphabet, p)) for p in equal] == [15] * 4
    for bias, stop in ((0.0, -1), (1.0, SPACE)):
        r, texts, nbytes, _ = score_and_continue(lib, net, alphabet, equal, seeds[:4], 1, 40, bias, stop, 400)
        r2, texts2, nbytes2 = char_continue_texts(lib, net, alphabet, equal, seeds[:4], 40, bias, stop, 400)
        assert r == 0 and r2 == 0 and texts == texts2 and nbytes == nbytes2
    # three passages per prompt, every prompt fed once: no launch more than for one passage per prompt, counted by the
    # library itself (rnn_amd_kernel_time_ms)
    lib.rnn_amd_kernel_time_enable(1)
    launches(lib)
    r1, once, _, ent1 = score_and_continue(lib, net, alphabet, equal, seeds[0:12:3], 1, 40, 0.0, -1, 400)
    n1 = launches(lib)
    r3, thrice, nbytes3, ent3 = score_and_continue(lib, net, alphabet, equal, seeds, 3, 40, 0.0, -1, 400)
    n3 = launches(lib)
    lib.rnn_amd_kernel_time_enable(0)
    print("launches by class, one passage per prompt", n1, "three", n3)
    # (the library times its forward GEMM, class 2: one launch per forward pass of a wave; the k_texts_* launches between
    # the passes are in no class.)  14 passes feed the prompts of 15 symbols, once; 40 continue from their last symbols:
    # were the prompts fed again in front of the draws it would be 14 + 54, and nothing grows with the passages
    assert r1 == 0 and r3 == 0 and n1[2] == 14 + 40 and n3 == n1
    assert np.array_equal(ent1, ent3) and len(once) == 4 and len(thrice) == 12
    assert all(len({thrice[3 * k], thrice[3 * k + 1], thrice[3 * k + 2]}) == 3 for k in range(4)) and nbytes3 == [40] * 12
    lib.rnn_char_free_alphabet(alphabet)
    lib.rnn_delete_net(net)


def test_the_tool_scores_and_continues_with_P_and_e(amd, tmp_path):
    lib = amd
    build = os.path.join(rc.ROOT, "build")
    path = str(tmp_path / "erewhon.net")
    r = subprocess.run([os.path.join(build, "text_predict_amd"), "-f", rc.EREWHON, "-H", "99", "-t", "16", "-d", "10",
                        "-l", "1e-3", "-s", "60", "-r", "60", "-V", "1500", "-n", path],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0 and os.path.exists(path), r.stderr[-2000:]
    lines = ["the higher", "It was a Long", "of"]
    with open(tmp_path / "prompts.txt", "w") as f:
        f.write(lines[0] + "\n\n" + lines[1] + "\r\n" + lines[2])
    tool = [os.path.join(build, "text_confabulate_amd"), "-f", path, "-n", "30", "-B", "1", "-P", str(tmp_path / "prompts.txt"),
            "-N", "2", "-r", "5"]

    def run(args):
        r = subprocess.run(tool + args, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.split("\n")

    out = run(["-e"])
    assert len(out) == 7 and out[6] == ""
    net = lib.rnn_load_net(path.encode())
    alphabet = lib.rnn_char_new_alphabet_from_net(net)
    r, want, _, entropy = score_and_continue(lib, net, alphabet, [p.encode() for p in lines], [5 + i for i in range(6)], 2, 30,
                                             1.0, -1, 30 * 4 + 5)
    assert r == 0 and len(set(want)) >= 5
    for i, o in enumerate(out[:6]):
        bits, _, rest = o.partition("\t")
        assert bits == "%.6f" % entropy[i // 2] and rest.encode() == lines[i // 2].encode() + want[i]
    assert 1.0 < entropy[1] < 8.0
    lib.rnn_char_free_alphabet(alphabet)
    lib.rnn_delete_net(net)
    # without -e nothing changes: the prompt and its continuation, no figure
    plain = run([])
    assert len(plain) == 7 and all(p.startswith(l) and "\t" not in p for p, l in zip(plain[0:6:2], lines))
