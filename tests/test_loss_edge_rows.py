"""The CPU half of the loss-edge tests (tests/loss_edge_cases.py, tests/test_gpu_loss_edges.py): the oracle is a sound
reference on the catalogue's rows (bit-equal to the compiled reference where that is built), the designed net gives exactly
the rows that were written into it, every GPU case's rows reach every branch that the issue names, and the rows would catch
each single-rule slip in the softmax (a numpy restatement, first held bit-equal to the oracle, then mutated)."""

import numpy as np
import pytest

import loss_edge_cases as le
import recur_ctypes as rc
import scenarios as sc

F = np.float32
BAR = 1e-4  # the GPU tests' bar on o_error and on the statistics


@pytest.fixture(scope="module")
def orc():
    return rc.load_oracle()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _lib_softmax_best_guess(fn, row):
    err = np.zeros(len(row), np.float32)
    best = fn(rc.fptr(err), rc.fptr(np.ascontiguousarray(row)), len(row))
    return err, best


def test_every_row_is_finite_and_bounded_at_every_length():
    for n in le.LENGTHS + (5, 7, 30, 256):
        for seed in (0, 1, 2):
            for name, row in le.rows(n, seed).items():
                assert row.dtype == np.float32 and row.shape == (n,) and np.isfinite(row).all(), (n, name)
                assert np.abs(row).max() <= le.MAX_LOGIT
    x = le.sigmoid_arguments()
    assert np.isfinite(x).all() and np.abs(x).max() == le.MAX_LOGIT
    with pytest.raises(AssertionError):
        le.checked(np.array([np.inf], np.float32))
    with pytest.raises(AssertionError):
        le.checked(np.array([np.nan], np.float32))


def test_the_numpy_restatement_equals_the_oracle_in_every_bit(orc):
    """softmax_best_guess, fast_expf through fast_sigmoid, and capped_log2f's two sides"""
    for n in le.LENGTHS + (5, 7, 30, 256):
        for name, row in le.rows(n).items():
            want, want_best = _lib_softmax_best_guess(orc.orc_softmax_best_guess, row)
            got, got_best = le.softmax_best_guess(row)
            assert np.array_equal(_bits(got), _bits(want)) and got_best == want_best, (n, name)
            assert np.isfinite(want).all()
    x = le.sigmoid_arguments()
    want = np.array([orc.orc_fast_sigmoid(float(v)) for v in x], np.float32)
    assert np.array_equal(_bits(le.fast_sigmoid(x)), _bits(want))
    for v in (0.0, 1e-31, 9.9e-31, 1.1e-30, 1e-20, 0.5):
        got, want = le.capped_log2f(v), F(orc.orc_capped_log2f(v))
        assert got == want or abs(got - want) <= 1e-6 * abs(want)  # (numpy's log2 against libm's)


@pytest.mark.skipif(not rc.have_ref(), reason="oracle/_ref/librecur_ref.so was not built (needs the reference's sources)")
def test_the_oracle_equals_the_compiled_reference_on_every_row(orc):
    ref = rc.load_ref()
    for n in le.LENGTHS:
        for name, row in le.rows(n).items():
            want, want_best = _lib_softmax_best_guess(ref.ref_softmax_best_guess, row)
            got, got_best = _lib_softmax_best_guess(orc.orc_softmax_best_guess, row)
            assert np.array_equal(_bits(got), _bits(want)) and got_best == want_best, (n, name)
    for v in le.sigmoid_arguments():
        a, b = F(orc.orc_fast_sigmoid(float(v))), F(ref.ref_fast_sigmoid(float(v)))
        assert _bits(a) == _bits(b), v


# ------------------------------------------------------------------ the designed net on the oracle --

def designed_oracle(input_size, hidden_size, output_size, S, D, symbol_rows, activation=rc.RELU):
    """an OracleSet whose weights are the designed net's, momentum and aux arrays zero, learn rate zero"""
    o = sc.OracleSet(input_size=input_size, hidden_size=hidden_size, output_size=output_size, S=S, D=D, learn_rate=0.0,
                     seed=3, activation=activation)
    a = o.arrays()
    ih, ho = le.designed_weights(o.I, o.H, o.O, hidden_size, symbol_rows)
    a["ih_w"][:] = ih
    a["ho_w"][:] = ho
    for k in ("ih_m", "ho_m", "ih_aux", "ho_aux"):
        a[k][:] = 0
    return o


@pytest.mark.parametrize("n", [42, 65, 300])
def test_the_designed_net_gives_the_written_rows_bit_for_bit(n):
    """after 1 step and after D + 2 steps (learn rate 0, WEIGHTED momentum: the weights stay what was written), every
    symbol on some stream, every o_error finite"""
    named = le.symbol_rows(n)
    S, D = len(named), 4
    o = designed_oracle(n, 64, n, S, D, [r for _, r in named])
    pairs = [(c, int(np.argmin(row))) for c, (_, row) in enumerate(named)]
    text, positions, plan = le.stream_text(pairs * (D + 2), S)
    assert len(positions) == D + 2
    w0 = {k: o.arrays()[k].copy() for k in ("ih_w", "ho_w")}
    for k, i in enumerate(positions):
        o.char_step(text, i, rc.WEIGHTED, 0.9)
        a = o.arrays()
        if k in (0, D + 1):
            for j, (c, t) in enumerate(plan[k]):
                assert np.array_equal(_bits(a["output"][j, :n]), _bits(named[c][1])), (k, named[c][0])
            assert np.isfinite(a["o_error"]).all()
            hid = a["hidden"]
            assert ((hid != 0).sum(axis=1) == 2).all()  # the bias and the symbol's unit
    for k in w0:
        assert np.array_equal(o.arrays()[k], w0[k])
    o.close()


# ------------------------------------------------------------------ what the GPU cases reach --

def _coverage_of(lengths):
    named = [(name, row) for n in lengths for name, row in le.symbol_rows(n)]
    return le.coverage(named)


def test_every_gpu_case_reaches_every_branch():
    """asserted, not printed: all four shift branches, loop counts 0 to 4, a denormal and a zero likelihood, a capped
    entropy and a tie, among the rows that each GPU case scores.  The class groups and the sigmoid kernels keep no entropy
    statistic: their table is the same without the cap, resp. the saturations of the sigmoid."""
    for n in le.TEXT_NARROW + le.TEXT_WIDE + le.ALONE:
        le.assert_full_coverage(_coverage_of([n]), "text / stand-alone %d" % n)
    for alen, heads in le.HEADS:
        full, triples, slots = le.head_case(alen, heads)
        own = {}
        for c, h, t in triples:
            own.setdefault((c, h), []).append(t)
        named = [slots[c][h] for (c, h) in own]
        pairs = [(k, t) for k, ch in enumerate(own) for t in own[ch]]
        assert {name for name, _ in named} == set(le.rows(alen)), "a catalogue row no stream scores as its own head"
        le.assert_full_coverage(le.coverage(named, pairs), "heads %d x %d" % (alen, heads))
    full, offsets, sizes, slots = le.group_case()
    named = [s for per in slots for s in per]
    got = le.coverage(named, [])
    got["capped"] = True  # (no entropy statistic in train_channel's loss)
    le.assert_full_coverage(got, "class groups")
    for g, n in enumerate(le.GROUP_SIZES):  # ... and every group size sees a shifted row on its own
        assert {le.branch_of(per[g][1])["branch"] for per in slots} >= ({"none", "hi", "room"} if n == 1 else
                                                                        {"none", "hi", "room", "limited"})
    targets = np.stack([le.group_targets(slots, k) for k in range(5)])
    assert (targets == -1).any() and (targets >= 0).any()
    for alen, heads in le.XENT:
        full, text, slots, _ = le.xent_case(alen, heads)
        sc_ = le.xent_scored(slots, text)
        named = [(name, row) for _, name, row, _ in sc_]
        got = le.coverage(named, [])
        likes = np.array([le.scored(row, t)["likelihood"] for _, _, row, t in sc_])
        got["capped"] = bool((likes < F(1e-30)).any())
        assert ((likes >= F(1e-30)) & (likes < F(1e-20))).any()  # ... and a likelihood that only the 1e-30 cap lets through
        assert all(le.xent_safe(l) for l in likes)
        le.assert_full_coverage(got, "cross entropy %d x %d" % (alen, heads))
    x = le.sigmoid_arguments()
    _, count = le.fast_expf(-x)
    a = le.fast_sigmoid(x)
    assert set(int(c) for c in count) >= {0, 1, 2, 3, 4, 5} and (a == 0).any() and (a == 1).any()
    assert ((a > 0) & (a < le.TINY)).any()  # a denormal answer
    for n in (3, le.SIGMOID_WIDTH):
        rows_ = np.array(le.sigmoid_case(n))
        assert set(_bits(x)) <= set(_bits(rows_[:, :n].ravel()))  # every argument (-0.0 too) is some symbol's output


def test_the_likelihood_condition_drops_targets_never_rows():
    """on the oracle every scored (row, target) has 1 - error >= 1e-5 or exactly 0"""
    dropped_all = []
    for n in sorted(set(le.TEXT_NARROW + le.TEXT_WIDE + le.ALONE + tuple(a for a, _ in le.HEADS))):
        named = le.symbol_rows(n)
        pairs, dropped = le.pairs_of(named)
        assert {c for c, _ in pairs} == set(range(len(named))), "a row lost all its targets"
        for c, t in pairs:
            l = F(1) - le.scored(named[c][1], t)["target_error"]
            assert l >= F(1e-5) or l == 0
        dropped_all += dropped
    print("dropped (row, length, target):", dropped_all)


# ------------------------------------------------------------------ the rows catch every single-rule slip --

def _differs(got, want):
    """by more than the GPU tests' bar (a NaN differs)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore"):
        return bool((~(np.abs(got - want) <= BAR * np.abs(want))).any())


def _caught_by(mutation):
    caught = []
    for n in sorted(set(le.TEXT_NARROW + le.TEXT_WIDE + le.ALONE)):
        for name, row in le.symbol_rows(n):
            for t in (int(np.argmax(row)), int(np.argmin(row)), 0, n - 1):
                want, got = le.scored(row, t), le.scored(row, t, mutation)
                if (_differs(got["error"], want["error"]) or got["hit"] != want["hit"]
                        or _differs(got["entropy"], want["entropy"]) or _differs(got["xent"], want["xent"])):
                    caught.append((n, name, t))
    return caught


@pytest.mark.parametrize("mutation", ["no_lo", "no_min", "highest_tie", "cap_1e20"])
def test_a_slip_in_one_rule_changes_a_catalogue_row_by_more_than_the_bar(mutation):
    """the pattern of test_the_oracle_sees_every_move: no `lo` branch, `min` dropped from the limited shift, the highest
    index on a tie, the cap at 1e-20 -- each must move an error row, a hit, an entropy or a cross-entropy term of some
    catalogue (row, target) past the bar the GPU tests hold"""
    caught = _caught_by(mutation)
    assert caught, "no catalogue row notices the mutation %s" % mutation
    names = {name for _, name, _ in caught}
    expect = {"no_lo": {"all_m1000", "limited", "lowered"}, "no_min": {"limited", "lowered"},
              "highest_tie": {"tie_3_40", "tie_3_65", "tie_5_70", "tie_1_129"}, "cap_1e20": {"m61_room"}}[mutation]
    assert expect <= names, (mutation, sorted(names))


def test_ge_50_for_gt_50_is_the_same_function():
    """`hi >= 50` for `hi > 50` cannot be caught by any row: at hi == 50 the first branch's shift is 50 - hi = 0, and the
    branches it pre-empts give min(-60 - lo, 0) = 0 (lo < -60) or 0.  The two rows at the boundary prove it here -- bit
    equality, with lo on either side of -60 -- and the float above 50 takes the first branch under both."""
    for n in (4, 42, 65, 300):
        r = le.rows(n)
        low = r["at_50"].copy()
        low[0] = -200.0
        for row in (r["at_50"], low, r["above_50"], r["plain"]):
            a, b = le.softmax_best_guess(row), le.softmax_best_guess(row, "ge_50")
            assert np.array_equal(_bits(a[0]), _bits(b[0])) and a[1] == b[1]
        assert le.softmax_shift(r["at_50"].min(), 50.0) == (0.0, "none")
        assert le.softmax_shift(low.min(), 50.0) == (0.0, "limited")
        assert le.softmax_shift(low.min(), 50.0, "ge_50") == (0.0, "hi")
        hi = r["above_50"].max()
        assert le.softmax_shift(0.0, hi) == (F(50) - hi, "hi") and F(50) - hi < 0
