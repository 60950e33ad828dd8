"""The library's one exponential asked of the rule itself (recur_amd/csrc/fast_exp_rule.h: what fast_expf_dev runs on the
device and ramd_fast_expf on the host) without a GPU: fast_exp_rule_harness.cpp is compiled with g++ alone and prints the
value and the number of scaling rounds of every float it is given.

On every finite float asked -- every exponent with 64 mantissas and more, both signs, both neighbours of +-0.2, the zeros,
the denormals, +-FLT_MAX -- value and rounds are the numpy restatement's (loss_edge_cases.fast_expf), the values the
oracle's and, where oracle/_ref is built, the reference's, bit for bit.  On an infinity or a NaN, where the reference's
loop does not end (so neither the oracle nor the reference is ever asked), the rule gives a quiet NaN in no rounds.  The
same program runs under AddressSanitizer and UndefinedBehaviorSanitizer, stand-alone.

Then the rows that are not finite (loss_edge_cases.nonfinite_rows): that each reaches the exponential with an infinite
argument -- the loop that did not end -- which branch of the shift it takes, that the restated losses are NaN throughout,
and that the net written from FINITE weights (designed_nonfinite_weights) answers each poisoned symbol with exactly its row
and every clean symbol with exactly what it answered before."""
import os
import subprocess

import numpy as np
import pytest

import loss_edge_cases as le
import recur_ctypes as rc

ROOT = rc.ROOT
CSRC = os.path.join(ROOT, "recur_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "fast_exp_rule_harness.cpp")
CXX = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
F = np.float32
FLT_MAX = np.finfo(np.float32).max


def build_harness(directory, extra=()):
    exe = os.path.join(str(directory), "fast_exp_rule_harness")
    subprocess.run(CXX + list(extra) + [SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("fast_exp_rule"))


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    """the same program under AddressSanitizer and UndefinedBehaviorSanitizer: it has its own main, so the runtimes are
    linked into it and nothing is preloaded"""
    return build_harness(tmp_path_factory.mktemp("fast_exp_rule_san"),
                         ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def ask(exe, tmp_path, values):
    """-> (values float32, rounds) of the harness"""
    path = str(tmp_path / "values.f32")
    np.ascontiguousarray(values, F).tofile(path)
    r = subprocess.run([exe, "values", path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.array(r.stdout.split(), np.uint64).reshape(-1, 2)
    assert len(got) == len(values)
    return got[:, 0].astype(np.uint32).view(F), got[:, 1].astype(np.int64)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def finite_arguments():
    """every exponent field 0 (zero and the denormals) to 254 with 64 random mantissas and the all-zeros and all-ones ones,
    both signs; the neighbours of +-0.2; what the loss tests' rows bring"""
    g = np.random.default_rng(21)
    exps = np.repeat(np.arange(255, dtype=np.uint32), 66)
    man = np.concatenate([g.integers(0, 1 << 23, (255, 64), dtype=np.uint32),
                          np.zeros((255, 1), np.uint32), np.full((255, 1), (1 << 23) - 1, np.uint32)], axis=1).ravel()
    pos = ((exps << 23) | man).astype(np.uint32)
    swept = np.concatenate([pos, pos | np.uint32(0x80000000)]).view(F)
    p2 = F(0.2)
    near = np.array([np.nextafter(p2, F(0)), p2, np.nextafter(p2, F(1))], F)
    named = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, le.TINY, -le.TINY, FLT_MAX, -FLT_MAX, 50.0, -60.0, -110.0,
                      1e4, -1e4], F)
    x = np.concatenate([named, near, -near, swept, le.sigmoid_arguments()]).astype(F)
    assert np.isfinite(x).all()
    return x


def nonfinite_arguments():
    """+-inf, and NaNs of both signs, quiet and signalling, with several payloads"""
    payloads = [1, 2, 0x155555, 0x2aaaaa, 0x3fffff]
    words = [0x7f800000, 0xff800000]
    for sign in (0, 0x80000000):
        words += [sign | 0x7fc00000] + [sign | 0x7fc00000 | p for p in payloads]       # quiet
        words += [sign | 0x7f800000 | p for p in payloads]                              # signalling
    return np.array(words, np.uint32).view(F)


def check_finite(exe, tmp_path):
    x = finite_arguments()
    got, rounds = ask(exe, tmp_path, x)
    want, want_rounds = le.fast_expf(x)
    assert np.array_equal(_bits(got), _bits(want)), x[_bits(got) != _bits(want)][:5]
    assert np.array_equal(rounds, want_rounds), x[rounds != want_rounds][:5]
    # what the arguments are there for: no round up to 0.2 (the comparison is made in double: the float 0.2 is above it),
    # one beyond, none for a denormal, and the most of all at FLT_MAX
    at = {int(b): int(r) for b, r in zip(_bits(x), rounds)}
    p2 = F(0.2)
    for s in (F(1), F(-1)):
        assert at[int(_bits(s * np.nextafter(p2, F(0)))[0])] == 0 and at[int(_bits(s * p2)[0])] == 1
        assert at[int(_bits(s * F(0))[0])] == 0 and at[int(_bits(s * F(1e-45))[0])] == 0
        assert at[int(_bits(s * FLT_MAX)[0])] == rounds.max() == want_rounds.max()
    assert set(range(int(rounds.max()) + 1)) == set(int(r) for r in rounds)   # every count up to the largest is met
    assert np.isfinite(got[x <= 0]).all() and (got[x == 0] == 1).all()
    return x, got, rounds


def check_nonfinite(exe, tmp_path):
    x = nonfinite_arguments()
    assert not np.isfinite(x).any() and np.isinf(x).sum() == 2 and len(x) > 20
    got, rounds = ask(exe, tmp_path, x)
    assert np.isnan(got).all() and (rounds == 0).all()
    assert ((_bits(got) & np.uint32(0x00400000)) != 0).all()                  # quiet
    want, want_rounds = le.fast_expf(x)
    assert np.isnan(want).all() and (want_rounds == 0).all()


def check_sweep(exe):
    """the largest count over the finite floats: the count never falls as |x| grows (asked of every 251st float), so it is
    FLT_MAX's, and that is the restatement's"""
    r = subprocess.run([exe, "sweep", "251"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    largest, descents, asked = (int(v) for v in r.stdout.split())
    assert descents == 0 and asked > 2 * (0x7f7fffff // 251)
    assert largest == int(le.fast_expf(FLT_MAX)[1][0]) == int(le.fast_expf(-FLT_MAX)[1][0])


def test_the_header_needs_no_hip_and_is_c_as_well():
    hdr = os.path.join(CSRC, "fast_exp_rule.h")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-x", "c++",
                    hdr], check=True)
    subprocess.run(["gcc", "-std=gnu11", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-x", "c", hdr],
                   check=True)


def test_there_is_one_scaling_loop_in_the_library():
    """the rule's header has it; no other file of recur_amd/csrc multiplies by 0.125 or compares with 0.2 in a loop's
    condition, and both callers' own functions are calls of the rule"""
    holders = []
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".h", ".c", ".hip", ".cpp")):
            text = open(os.path.join(CSRC, name)).read()
            if "*= 0.125" in text or "> 0.2)" in text:
                holders.append(name)
    assert holders == ["fast_exp_rule.h"], holders
    assert "float fast_expf_dev(float x) { return fast_expf(x); }" in open(os.path.join(CSRC, "k_top.h")).read()
    assert "float ramd_fast_expf(float x) { return fast_expf(x); }" in open(os.path.join(CSRC, "rnn_init.c")).read()


def test_finite_arguments_are_the_restatement_and_the_oracle_bit_for_bit(harness, tmp_path):
    x, got, _ = check_finite(harness, tmp_path)
    orc = rc.load_oracle()
    want = np.array([orc.orc_fast_expf(float(v)) for v in x], F)       # finite arguments only: the oracle's loop is badmaths.h's
    assert np.array_equal(_bits(got), _bits(want))
    # and it IS an exponential where float32 can hold one: the Pade form's error after the squarings
    mid = np.abs(x) <= 80
    assert np.abs(got[mid].astype(np.float64) / np.exp(x[mid].astype(np.float64)) - 1).max() < 1e-3


@pytest.mark.skipif(not rc.have_ref(), reason="oracle/_ref/librecur_ref.so was not built (needs the reference's sources)")
def test_finite_arguments_are_the_references_fast_expf_bit_for_bit(harness, tmp_path):
    ref = rc.load_ref()
    x = finite_arguments()
    got, _ = ask(harness, tmp_path, x)
    want = np.array([ref.ref_fast_expf(float(v)) for v in x], F)
    assert np.array_equal(_bits(got), _bits(want))


def test_the_largest_round_count_is_the_restatements(harness):
    check_sweep(harness)


def test_what_is_not_finite_is_nan_in_no_rounds(harness, tmp_path):
    check_nonfinite(harness, tmp_path)


def test_under_address_and_undefined_behaviour_sanitizers(sanitized, tmp_path):
    """stand-alone: the harness has its own main, the sanitizers' runtimes are linked into it"""
    check_finite(sanitized, tmp_path)
    check_nonfinite(sanitized, tmp_path)
    check_sweep(sanitized)


# ------------------------------------------------------------------ the rows that are not finite --

WIDTHS = (2, 3, 5, 7, 30, 42, 64, 65, 73, 128, 130, 300)


def test_every_such_row_reaches_the_loop_that_did_not_end():
    """per row: the shift's branch, that an argument arrives infinite (`nan`: as a NaN, which ended the loop before and is
    pinned all the same), and what the restated losses make of it -- NaN throughout"""
    for n in WIDTHS:
        r = le.nonfinite_rows(n)
        assert set(r) == {"pos_inf", "neg_inf", "both", "nan"} | ({"pos_inf_late"} if n > 64 else set()), n
        p, q = n // 2, (n // 2 + 1) % n
        assert np.array_equal(le.nonfinite_rows(n)["pos_inf"][np.arange(n) != p], le.rows(n)["plain"][np.arange(n) != p])
        for name, row in r.items():
            assert row.dtype == np.float32 and row.shape == (n,)
            branch, arg = le.arrivals(row)
            bad = ~np.isfinite(row)
            want_branch = {"pos_inf": "hi", "pos_inf_late": "hi", "both": "hi", "neg_inf": "limited", "nan": "none"}[name]
            assert branch == want_branch, (n, name, branch)
            if name == "nan":
                assert bad.sum() == 1 and np.isnan(row[p]) and np.isnan(arg[p]) and np.isfinite(np.delete(arg, p)).all()
            elif name == "neg_inf":
                assert np.isneginf(row[p]) and np.isneginf(arg[p]) and np.isfinite(np.delete(arg, p)).all()
            else:
                where = n - 1 if name == "pos_inf_late" else p
                assert np.isposinf(row[where]) and np.isnan(arg[where])          # inf - inf
                rest = np.delete(arg, where)
                assert np.isneginf(rest).all() and len(rest) >= 1                 # every finite entry, and `both`'s -inf
                if name == "both":
                    assert np.isneginf(row[q])
            assert np.isinf(arg).any() or name == "nan"
            ex, rounds = le.fast_expf(arg)
            assert np.isnan(ex[~np.isfinite(arg)]).all() and (rounds[~np.isfinite(arg)] == 0).all()
            for t in sorted({0, p, n - 1, int(np.argmin(np.where(bad, np.inf, row)))}):
                s = le.scored(row, t)
                assert np.isnan(s["error"]).all() and np.isnan(s["target_error"]) and np.isnan(s["likelihood"])
                assert np.isnan(s["entropy"]) and np.isnan(s["xent"])           # NaN < 1e-30 is false: log2 of a NaN
            sig = le.fast_sigmoid(row)
            assert np.array_equal(np.isnan(sig), bad), (n, name)                 # elementwise: the others are what they were
            assert np.array_equal(_bits(sig[~bad]), _bits(le.fast_sigmoid(le.rows(n)["plain"])[~bad]))


@pytest.mark.parametrize("n", [5, 42, 65, 130, 300])
def test_finite_weights_give_exactly_these_rows_and_leave_the_clean_ones_alone(n):
    """a float32 forward pass of the written net: each poisoned symbol's output row is the catalogue's, an infinity by its
    bits and a NaN where a NaN is; every clean symbol's row and hidden row are what the all-clean net's are, bit for bit"""
    clean = [r for _, r in le.symbol_rows(n)][:6]
    bad = list(le.nonfinite_rows(n).items())
    hidden_size = 64
    I, H, O = 1 + hidden_size + max(n, 16), hidden_size + 4, n + 3
    rows_ = clean + [r for _, r in bad]
    ih, ho = le.designed_nonfinite_weights(I, H, O, hidden_size, rows_)
    assert np.isfinite(ih).all() and np.isfinite(ho).all() and np.abs(ho).max() == le.HUGE
    ih0, ho0 = le.designed_weights(I, H, O, hidden_size, clean)
    for c, row in enumerate(clean):
        hid, out = le.designed_forward(ih, ho, hidden_size, c)
        hid0, out0 = le.designed_forward(ih0, ho0, hidden_size, c)
        assert np.array_equal(_bits(out), _bits(out0)) and np.array_equal(_bits(hid), _bits(hid0))
        assert np.array_equal(_bits(out[:n]), _bits(row)) and not out[n:].any()
    for k, (name, row) in enumerate(bad):
        hid, out = le.designed_forward(ih, ho, hidden_size, len(clean) + k)
        nan = np.isnan(row)
        assert np.array_equal(np.isnan(out[:n]), nan), name
        assert np.array_equal(_bits(out[:n][~nan]), _bits(row[~nan])), name
        assert np.isfinite(hid).all() and hid.max() == 2.0 and (hid != 0).sum() == (3 if nan.any() else 2)
        assert not out[n:].any()
    with pytest.raises(AssertionError):                                           # no room for the NaN's own unit
        le.designed_nonfinite_weights(I, H, O, len(rows_), rows_)
