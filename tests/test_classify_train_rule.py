"""What gstclassify's trainer decides per generation, asked of the rule itself (recur_amd/csrc/classify_train_rule.h: what
rnn_amd_set_classify_steps, rnn_amd_classify_generations and the gate of the loss kernels follow) without a GPU:
classify_train_rule_harness.cpp is compiled with g++ alone and prints the masks, active counts and generation counters of a
block, the gate of a wrongness, the refusals and the balanced-training choice.  The expected values are
tests/classify_train_cases.py's numpy restatement and must be met exactly.  The restatement is then broken one rule at a time,
and each broken form must differ on these inputs: the device tests, which hold the call to the same restatement, would
notice that rule being wrong."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import classify_train_cases as cc
import recur_ctypes as rc

ROOT = rc.ROOT
CSRC = os.path.join(ROOT, "recur_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "classify_train_rule_harness.cpp")
CXX = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
F = np.float32


def build(tmp_path_factory, name, extra=()):
    exe = str(tmp_path_factory.mktemp(name) / "classify_train_rule_harness")
    subprocess.run(CXX + list(extra) + [SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build(tmp_path_factory, "classify_train_rule")


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    """the same program under AddressSanitizer and UndefinedBehaviorSanitizer: it has its own main, so the runtimes are
    linked into it and nothing is preloaded"""
    return build(tmp_path_factory, "classify_train_rule_san", ["-O1", "-g", "-fsanitize=address,undefined",
                                                               "-fno-sanitize-recover=all"])


def ask(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def commas(a):
    return ",".join(str(int(v)) for v in a)


def test_the_header_needs_no_hip_and_is_c_as_well():
    hdr = os.path.join(CSRC, "classify_train_rule.h")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-x", "c++",
                    hdr], check=True)
    subprocess.run(["gcc", "-std=gnu11", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-x", "c", hdr],
                   check=True)


# ------------------------------------------------------------------ masks, active counts, generation counters --

def blocks():
    """(name, targets [T][n][G], sizes): random blocks on the three group shapes, stream counts that are and are not a
    whole number of words, and the designed rows"""
    out = [("designed", cc.designed_targets(), cc.GAP[1])]
    for k, (n, groups) in enumerate(((1, cc.ONE_OF_2), (3, cc.GAP), (4, cc.WIDE), (64, cc.ONE_OF_2), (130, cc.GAP))):
        out.append(("random %d" % n, cc.block_of(5, n, 4, groups, 50 + k, silent=(3,))[1], groups[1]))
    return out


def harness_decisions(exe, directory, tg, sizes, gen0=7):
    path = os.path.join(str(directory), "targets.i32")
    np.ascontiguousarray(tg, np.int32).tofile(path)
    T, n, G = tg.shape
    v = np.array(ask(exe, "decisions", T, n, G, commas(sizes), gen0, path).split(), np.int64)
    stride = (n + 3) & ~3
    return v[:T * stride].reshape(T, stride), v[T * stride:T * stride + T], v[T * stride + T:-1], int(v[-1])


def check_decisions(exe, directory):
    for name, tg, sizes in blocks():
        masks, active, gen, trained = harness_decisions(exe, directory, tg, sizes)
        want_masks, want_active, want_gen = cc.np_decisions(tg, sizes, generation=np.full(tg.shape[1], 7))
        assert np.array_equal(masks, want_masks) and np.array_equal(active, want_active), name
        assert np.array_equal(gen, want_gen), name
        assert trained == int(cc.np_trains(tg, sizes).sum()), name
        assert (masks[:, tg.shape[1]:] == 0).all(), "the padding of a mask is clear"


def test_decisions_are_the_restatement(harness, tmp_path):
    named = blocks()
    assert {tg.shape[1] % 4 for _, tg, _ in named} == {0, 1, 2, 3}
    check_decisions(harness, tmp_path)
    # the designed rows: a label equal to the size, one past it and INT_MIN are no labels; a generation has none at all
    masks, active, gen = cc.np_decisions(cc.designed_targets(), cc.GAP[1])
    assert masks[0, :11].tolist() == [1, 1, 1, 1, 0, 1, 1, 0, 0, 0, 1] and active.tolist() == [7, 7, 0, 7]
    assert gen.tolist() == [int(masks[:, j].sum()) for j in range(11)] and 0 < gen.min() < gen.max() == 3


@pytest.mark.parametrize("broken", ["active_on_any_non_negative", "generation_for_inactive"])
def test_each_decision_rule_is_noticed(broken):
    differ = 0
    for name, tg, sizes in blocks():
        right, wrong = cc.np_decisions(tg, sizes), cc.np_decisions(tg, sizes, broken=broken)
        differ += not all(np.array_equal(a, b) for a, b in zip(right, wrong))
    assert differ >= 2, broken


# ------------------------------------------------------------------ the gate --

def gate_bits():
    return [int(np.array([v], F).view(np.uint32)[0]) for _, v, _ in cc.GATE_VALUES]


def check_gate(exe):
    got = [int(v) for v in ask(exe, "gate", *gate_bits()).split()]
    assert got == [w for _, _, w in cc.GATE_VALUES]
    assert got == [int(cc.np_gate_raises(v)) for _, v, _ in cc.GATE_VALUES]


def test_the_gate_on_zeros_denormals_one_infinity_and_nan(harness):
    names = [n for n, _, _ in cc.GATE_VALUES]
    assert {"zero", "minus zero", "smallest denormal", "one", "infinity", "NaN"} <= set(names)
    check_gate(harness)


def test_a_gate_on_trained_is_noticed():
    """raised whenever a stream trained, in place of wrongness: differs on the two zeros, which is the certain classifier"""
    differ = [n for n, v, _ in cc.GATE_VALUES if cc.np_gate_raises(v, broken="gate_on_trained") != cc.np_gate_raises(v)]
    assert differ == ["zero", "minus zero"]


# ------------------------------------------------------------------ the refusals --

def check_refusals(exe):
    texts = {}
    for name, (hf, ht, steps, ld, n_in, G, offsets, sizes, n_out), want in cc.REFUSALS:
        out = ask(exe, "refusal", hf, ht, steps, ld, n_in, G, "-" if offsets is None else commas(offsets),
                  "-" if sizes is None else commas(sizes), n_out)
        code, text = out.strip().split(" ", 1)
        assert int(code) == want, name
        texts.setdefault(want, set()).add(text)
    assert set(texts) == set(range(6))
    assert all(len(t) == 1 for t in texts.values()) and len({next(iter(t)) for t in texts.values()}) == 6      # a text each


def test_every_refusal_and_the_blocks_it_takes(harness):
    check_refusals(harness)


# ------------------------------------------------------------------ the balanced choice --

def test_the_restated_generator_is_the_oracles():
    orc = rc.load_oracle()
    rng = rc.OrcRng()
    orc.orc_init_rand64(C.byref(rng), 12345)
    mine = cc.Jenkins(rng.a, rng.b, rng.c, rng.d)
    assert [mine.rand64() for _ in range(50)] == [orc.orc_rand64(C.byref(rng)) for _ in range(50)]


def test_the_probabilities_are_the_librarys_and_the_restatements(harness):
    """classify_balance_probabilities is what rnn_amd_balanced_begin calls: the library's figures (host code, no device),
    the header's under g++ and numpy's agree bit for bit"""
    lib = rc.bind_classify(rc.load_amd())
    for bias in (0.5, 1.0, 1.5, 3.0):
        for seen in ([0, 0, 0], [5, 0, 1], [1000, 3, 0, 77], [2 ** 31, 2 ** 31 - 5, 9]):      # (the sum wraps, as a u32 does)
            b = lib.rnn_amd_balanced_new(len(seen), bias)
            for k, v in enumerate(seen):
                b.contents.seen[k] = v
            lib.rnn_amd_balanced_begin(b)
            library = np.array(b.contents.train_p[:len(seen)], F)
            lib.rnn_amd_balanced_free(b)
            got = np.array(ask(harness, "probabilities", int(np.array([bias], F).view(np.uint32)[0]), commas(seen)).split(),
                           np.int64).astype(np.uint32)
            want = cc.np_train_p(seen, bias)
            assert np.array_equal(got, library.view(np.uint32)), (bias, seen)
            assert np.array_equal(got, want.view(np.uint32)), (bias, seen, got.view(F), want)


def choice_case():
    groups = cc.GAP
    tg = cc.block_of(6, 9, 4, groups, 60)[1]
    tg[:, :, 0] = np.where(tg[:, :, 0] == 1, 0, tg[:, :, 0])      # (a common class: its probability falls)
    return groups, tg, cc.Jenkins(0xf1ea5eed, 99, 99, 99)


def harness_choice(exe, directory, groups, tg, draws, bias):
    tpath, dpath = os.path.join(str(directory), "targets.i32"), os.path.join(str(directory), "draws.u64")
    np.ascontiguousarray(tg, np.int32).tofile(tpath)
    np.array(draws, np.uint64).tofile(dpath)
    T, n, G = tg.shape
    lines = ask(exe, "choose", T, n, G, commas(groups[0]), commas(groups[1]), groups[2],
                "-" if bias is None else int(np.array([bias], F).view(np.uint32)[0]), tpath, dpath).strip().splitlines()
    per = [np.array(ln.split(), np.int64) for ln in lines[:-1]]
    last = np.array(lines[-1].split(), np.int64)
    return per, last[:groups[2]], last[groups[2]:2 * groups[2]], int(last[-1])


def restated_choice(groups, tg, gen, bias, broken=None):
    seen, used = np.zeros(groups[2], np.uint32), np.zeros(groups[2], np.uint32)
    draws = iter(gen.rand64, None)
    per, taken = [], 0
    for t in range(tg.shape[0]):
        p = cc.np_train_p(seen, bias)
        use, trains, k = cc.np_choose(tg[t], groups[0], groups[1], p, seen, used, draws, broken)
        taken += k
        per.append(np.concatenate([use.reshape(-1), trains, [int((use >= 0).sum())]]))
    return per, seen, used, taken


def check_choice(exe, directory):
    groups, tg, gen = choice_case()
    stream = cc.Jenkins(*gen.s)
    draws = [stream.rand64() for _ in range(tg.size)]
    per, seen, used, taken = harness_choice(exe, directory, groups, tg, draws, 1.5)
    wper, wseen, wused, wtaken = restated_choice(groups, tg, gen, 1.5)
    assert all(np.array_equal(a, b) for a, b in zip(per, wper)) and len(per) == len(wper)
    assert np.array_equal(seen, wseen) and np.array_equal(used, wused) and taken == wtaken
    assert taken == int(cc.np_trains(tg, groups[1]).sum()), "one draw per labelled pair"
    assert 0 < used.sum() < seen.sum(), "the draw left nothing out: the case shows nothing"
    # without balance every label trains and nothing is drawn or counted
    per, seen, used, taken = harness_choice(exe, directory, groups, tg, draws, None)
    assert taken == 0 and not seen.any() and not used.any()
    for t, line in enumerate(per):
        want = np.where(cc.np_trains(tg[t], groups[1]), tg[t], -1)
        assert np.array_equal(line[:want.size], want.reshape(-1)) and line[-1] == (want >= 0).sum()


def test_the_balanced_choice_is_the_restatement(harness, tmp_path):
    check_choice(harness, tmp_path)


def test_draws_in_group_major_order_are_noticed():
    groups, tg, gen = choice_case()
    right = restated_choice(groups, tg, cc.Jenkins(*gen.s), 1.5)
    wrong = restated_choice(groups, tg, cc.Jenkins(*gen.s), 1.5, broken="draws_group_major")
    assert right[3] == wrong[3], "the same number of draws"
    assert not all(np.array_equal(a, b) for a, b in zip(right[0], wrong[0]))


def test_every_broken_form_has_its_test():
    assert set(cc.BROKEN) == {"active_on_any_non_negative", "gate_on_trained", "generation_for_inactive", "draws_group_major"}


def test_under_address_and_undefined_behaviour_sanitizers(sanitized, tmp_path):
    """stand-alone: the harness has its own main, the sanitizers' runtimes are linked into it"""
    check_decisions(sanitized, tmp_path)
    check_gate(sanitized)
    check_refusals(sanitized)
    check_choice(sanitized, tmp_path)
