"""Whether a forward pass may take the presynaptic noise that was generated ahead of it, asked of the rule itself
(recur_amd/csrc/noise_ahead.h, what noise_ahead.c, the set API's files and engine.c ask) without a GPU: noise_ahead_harness.cpp is
compiled with g++ alone, is fed events and prints the rule's answer to each.

The rule counts the events that move a generator and compares counts.  The model it is held to here compares HISTORIES:
the true generator state is the tuple of everything that has moved the generators since the start -- a host write is a
token of its own, a pass is ("pass", rows, level), a loss is ("loss", draws per stream), where a stream draws once per head
but its own (so `heads` times when its class is none of them).  A slot's content is the history its values start from and
the history its states stand for.  A launch from the generators starts at the true history (it is ordered behind the main
stream's work); a launch from a slot's states starts at what that slot holds when the side stream gets there, with the loss
the classes on the device cause, or with `skip` draws per stream, added.  A pass may adopt a slot only if its start IS the
true history, for the pass's rows and level.

What the model takes from the callers (set_loss.c, set_train.c) rather than from the rule: an offer between a pass and its loss is
followed by that loss, of that many heads, with no upload in between -- both are one call (rnn_amd_set_multi_step_deltas);
the sets of one engine that train with classes are equally wide here and the classes on the device are those of the last
upload, the engine's one in-range flag being what the rule keeps; and a class is in range, or stray, for either head count.
(Outside this model, and not changed by stating the rule once: a set that steps on with classes it uploaded earlier, one of
them stray, after ANOTHER set of the engine has uploaded classes that are all heads.  The flag then speaks of the other
set's classes, and a slot filled two ahead for the first set is kept although its assumption fails.)"""
import os
import random
import subprocess
from collections import Counter

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "recur_amd", "csrc")
A, B = (0, 4), (4, 4)           # two sets of one engine: (row0, n)
LEVELS = (0.02, 0.05)
HEADS = (2, 3)
GOOD = (0, 1, 1, 0)             # one of the heads, for either head count
STRAY = (0, 1, 7, 0)            # stream 2's class is none of them
GENERATORS = -1


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("noise_ahead") / "noise_ahead_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "noise_ahead_harness.cpp"), "-o", exe], check=True)
    return exe


def test_the_header_is_plain_c_and_cxx_without_hip():
    subprocess.run(["g++", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-x", "c++",
                    os.path.join(CSRC, "noise_ahead.h")], check=True)
    subprocess.run(["gcc", "-std=gnu11", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-x", "c",
                    os.path.join(CSRC, "noise_ahead.h")], check=True)   # (noise_ahead.c, the set API's files and engine.c are C)


class Rule:
    """the harness as a process that is asked event by event, the model beside it; every answer is held to the model as it
    comes, and `log` keeps (event, answer) for the tests that look at a sequence as a whole"""

    def __init__(self, exe, mode):
        self.mode = mode
        self.proc = subprocess.Popen([exe, str(mode)], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1)
        self.hist = ()                  # the true generator state
        self.slot = [None, None]        # dict(start, after, rows, level) or None: never filled, or freed
        self.stamp = [None, None]       # (version, assumed_classes) of the slot's last launch
        self.classes = None             # on the device
        self.tokens = 0
        self.state = dict(moves=0, head=0, adopted=-1, in_range=0, pending="00")
        self.counts = Counter()
        self.log = []

    def close(self):
        self.proc.stdin.close()
        assert self.proc.wait() == 0

    def ask(self, *words):
        self.proc.stdin.write(" ".join(str(w) for w in words) + "\n")
        self.proc.stdin.flush()
        fields = self.proc.stdout.readline().split()
        assert fields and fields[0] == words[0], (words, fields)
        ans = {"launch": []}
        for f in fields[1:]:
            k, v = f.split("=")
            if k == "launch":
                ans["launch"].append(tuple(int(x) for x in v.split(",")))
            else:
                ans[k] = v if k == "pending" else int(v)
        before, self.state = self.state, {k: ans[k] for k in ("moves", "head", "adopted", "in_range", "pending")}
        self.log.append((words, ans))
        return before, ans

    def pending(self, k, state=None):
        return (state or self.state)["pending"][k] == "1"

    def draws(self, heads):
        return tuple(heads - (0 <= c < heads) for c in self.classes)

    # ---- the events ----
    def write(self):
        self.ask("write")
        self.tokens += 1
        self.hist += (("write", self.tokens),)
        assert self.state["pending"] == "00"

    def free(self):
        self.ask("free")
        self.slot = [None, None]
        assert self.state["pending"] == "00" and self.state["adopted"] == -1

    def upload(self, heads, classes):
        self.ask("classes", heads, *classes)
        self.classes = tuple(classes)
        assert self.state["in_range"] == int(all(0 <= c < heads for c in classes))

    def forward(self, rows, level, bottom=0):
        """-> the slot the pass took, or -1"""
        before, ans = self.ask("pass", rows[0], rows[1], level, bottom)
        took, k = ans["took"], before["head"]
        assert took == self.state["adopted"]
        if level == 0:
            assert took == -1 and self.state["moves"] == before["moves"] and self.state["pending"] == before["pending"]
            return took
        assert self.state["moves"] == before["moves"] + 1
        if took >= 0:                                   # soundness: the values start where the generators stand
            s = self.slot[took]
            assert took == k and self.pending(k, before) and not bottom
            assert s is not None and s["start"] == self.hist, (s, self.hist)
            assert s["rows"] == rows and s["level"] == level
            assert self.state["head"] == k ^ 1 and not self.pending(k)
            assert self.pending(k ^ 1) == self.pending(k ^ 1, before)       # the one further ahead stays
            self.counts["adopted"] += 1
        else:
            assert self.state["pending"] == "00" and self.state["head"] == k
            if self.pending(k, before):                 # refused: the model has to know why
                s = self.slot[k]
                cause = ("bottom" if bottom else "rows" if s["rows"] != rows else "level" if s["level"] != level else
                         "version" if s["start"] != self.hist else None)
                assert cause, ("refused what the model would have taken", s, self.hist)
                self.counts["refused: " + cause] += 1
        self.hist += (("pass", rows, level),)
        return took

    def offer(self, rows, level, loss_classes=0):
        """-> the launches [(dst, src, n_classes, skip, version, assumed_classes)]"""
        before, ans = self.ask("offer", rows[0], rows[1], level, loss_classes)
        launches = ans["launch"]
        assert ans["behind_main"] == (1 if launches else 0)    # whatever it fills or reads: behind the main stream's work
        assert self.state["moves"] == before["moves"] and self.state["head"] == before["head"]
        if self.mode == 0 or level == 0 or (loss_classes and before["adopted"] < 0):
            assert not launches
        for i, (dst, src, n_classes, skip, version, assumed) in enumerate(launches):
            assert not self.pending(dst, before), "a slot that is pending is filled again"
            # the slot the current pass adopted may be filled again only behind that pass: behind_main (above); a slot
            # read after an earlier launch of this offer wrote it is meant to be read so: its stamp builds on the new one
            for d2, _, _, _, v2, _ in launches[:i]:
                assert dst != d2
                if src == d2:
                    assert version == v2 + 2
            if src == GENERATORS:
                assert n_classes == 0 and skip == 0 and assumed == 0
                start = self.hist
            else:
                held = self.slot[src]
                assert held is not None, "a launch from states that were never generated"
                n = rows[1]
                assert not (n_classes and skip) and (assumed == 0 if n_classes else skip == assumed - 1)
                start = held["after"] + (("loss", self.draws(n_classes) if n_classes else (skip,) * n),)
            assert version == len(start)        # every token of a history is one move
            self.slot[dst] = dict(start=start, after=start + (("pass", rows, level),), rows=rows, level=level)
            self.stamp[dst] = (version, assumed)
            assert self.pending(dst)
            self.counts["launches"] += 1
        return launches

    def loss(self, heads):
        """-> whether the rule dropped what was generated ahead"""
        before, ans = self.ask("loss", heads)
        assert self.state["moves"] == before["moves"] + 1
        hit = [self.stamp[k] for k in range(2)
               if self.pending(k, before) and self.stamp[k][1] and self.stamp[k][0] == self.state["moves"]]
        if ans["dropped"]:
            assert hit and self.state["pending"] == "00"
            stray = any(not 0 <= c < heads for c in self.classes)
            cause = "assumed classes" if any(a != heads for _, a in hit) else "stray class" if stray else None
            assert cause, "dropped noise whose assumption held"
            self.counts["dropped: " + cause] += 1
        else:
            assert self.state["pending"] == before["pending"]
        self.hist += (("loss", self.draws(heads)),)
        return ans["dropped"]

    # ---- the callers' sequences (set_loss.c, set_train.c) ----
    def text_step(self, rows, level):
        """char_step_deltas: the pass, then the offer -- no draws between this pass's noise and the next one's"""
        took = self.forward(rows, level)
        return took, self.offer(rows, level)

    def multi_calls(self, rows, level, heads, classes=GOOD):
        """rnn_amd_set_multi_text_loss: the pass, then the loss with its classes and the offer behind it"""
        took = self.forward(rows, level)
        self.upload(heads, classes)
        self.loss(heads)
        return took, self.offer(rows, level)

    def multi_step(self, rows, level, heads, classes=GOOD):
        """multi_step_deltas: the classes, the pass, the early offer if the pass adopted -- at its seam or right behind it
        -- and the loss; the plain offer behind the loss only if no early one was made"""
        if classes is not None:
            self.upload(heads, classes)
        took = self.forward(rows, level)
        launches = self.offer(rows, level, heads) if took >= 0 else None
        dropped = self.loss(heads)
        if launches is None:
            launches = self.offer(rows, level)
        return took, launches, dropped


@pytest.fixture
def rule(harness):
    made = []

    def make(mode):
        made.append(Rule(harness, mode))
        return made[-1]
    yield make
    for r in made:
        r.close()


# ------------------------------------------------------------------------------------------------ soundness

def random_events(r, rng, n_events):
    heads = rng.choice(HEADS)
    r.upload(heads, GOOD)
    rows, level = A, LEVELS[0]
    for _ in range(n_events):
        # a caller mostly goes on with the set, the level and the head count it has
        if rng.random() < 0.12:
            rows = rng.choice((A, B))
        if rng.random() < 0.08:
            level = rng.choice(LEVELS)
        if rng.random() < 0.08:
            heads = rng.choice(HEADS)
        what = rng.choices(("multi_step", "multi_calls", "text_step", "pass", "pass0", "offer", "upload", "loss", "write",
                            "free"), (40, 6, 8, 4, 3, 4, 3, 3, 3, 1))[0]
        classes = STRAY if rng.random() < 0.15 else GOOD
        if what == "multi_step":
            r.multi_step(rows, level, heads, classes if rng.random() < 0.9 else None)
        elif what == "multi_calls":
            r.multi_calls(rows, level, heads, classes)
        elif what == "text_step":
            r.text_step(rows, level)
        elif what == "pass":
            r.forward(rows, level)
        elif what == "pass0":
            r.forward(rows, 0.0)
        elif what == "offer":
            r.offer(rows, level)
        elif what == "upload":
            r.upload(heads, classes)
        elif what == "loss":
            r.loss(heads)
        elif what == "write":
            r.write()
        else:
            r.free()


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_whatever_is_adopted_starts_where_the_generators_stand(rule, mode):
    counts = Counter()
    for seed in range(6):
        r = rule(mode)
        random_events(r, random.Random(1000 * mode + seed), 500)
        counts += r.counts
    print(mode, dict(counts))
    if mode == 0:
        assert not counts["adopted"] and not counts["launches"]
        return
    want = ["adopted", "refused: version", "refused: rows", "refused: level"]
    if mode == 2:       # (only a slot filled two ahead assumes anything)
        want += ["dropped: assumed classes", "dropped: stray class"]
    for k in want:
        assert counts[k] > 0, (k, dict(counts))


# ------------------------------------------------------------------------------------------------ the regular sequences

@pytest.mark.parametrize("mode", [0, 1, 2])
def test_text_steps_adopt_from_the_second_pass_on(rule, mode):
    r = rule(mode)
    for g in range(1, 9):
        took, launches = r.text_step(A, 0.05)
        assert (took >= 0) == (mode != 0 and g >= 2)
        assert len(launches) == (1 if mode else 0)
        assert all(l[1] == GENERATORS for l in launches)


@pytest.mark.parametrize("mode", [1, 2])
def test_separate_multi_head_calls_adopt_from_the_second_pass_on(rule, mode):
    r = rule(mode)
    for g in range(1, 9):
        took, launches = r.multi_calls(A, 0.02, 3)
        assert (took >= 0) == (g >= 2)
        assert [l[1:4] for l in launches] == [(GENERATORS, 0, 0)]


def test_the_one_call_multi_head_step_two_ahead(rule):
    r = rule(2)
    heads = 3
    for g in range(1, 10):
        moves = r.state["moves"]
        took, launches, dropped = r.multi_step(A, 0.02, heads)
        assert not dropped
        if g == 1:      # generates for itself and offers after its loss
            assert took == -1 and [l[1:] for l in launches] == [(GENERATORS, 0, 0, moves + 2, 0)]
            continue
        assert took >= 0
        # the offer came after the pass: the count stood at moves + 1
        early = (took ^ 1, took, heads, 0, moves + 2, 0)               # the next pass: from the adopted states, past this loss
        two = (took, took ^ 1, 0, heads - 1, None, heads)              # the one after: from the next one's, past the next loss
        if g == 2:
            assert launches[0] == early and len(launches) == 2
            assert launches[1] == two[:4] + (launches[0][4] + 2,) + two[5:]
        else:           # the next pass's slot is there already
            assert len(launches) == 1 and launches[0][:4] == two[:4] and launches[0][5] == heads
            assert launches[0][4] == moves + 2 + 2      # head's stamp: behind this loss; the other's two on


def test_the_one_call_multi_head_step_one_ahead(rule):
    r = rule(1)
    for g in range(1, 9):
        moves = r.state["moves"]
        took, launches, dropped = r.multi_step(A, 0.02, 2)
        assert (took >= 0) == (g >= 2) and not dropped and len(launches) == 1
        assert launches[0][1:] == ((took, 2, 0, moves + 2, 0) if g >= 2 else (GENERATORS, 0, 0, moves + 2, 0))


@pytest.mark.parametrize("g_bad", [3, 4, 6])
@pytest.mark.parametrize("how", ["stray class", "other head count"])
def test_an_assumption_that_fails_costs_one_pass(rule, g_bad, how):
    r = rule(2)
    for g in range(1, g_bad + 4):
        heads = 2 if how == "other head count" and g == g_bad else 3
        classes = STRAY if how == "stray class" and g == g_bad else GOOD
        n_before = len(r.log)
        took, launches, dropped = r.multi_step(A, 0.02, heads, classes)
        events = [w[0] for w, _ in r.log[n_before:]]
        if g == g_bad:
            assert took >= 0 and dropped and r.state["pending"] == "00"
            assert events == ["classes", "pass", "offer", "loss"]            # no offer follows that loss
        elif g == g_bad + 1:
            assert took == -1 and not dropped                                # generates for itself
            assert events == ["classes", "pass", "loss", "offer"] and len(launches) == 1
        else:
            assert (took >= 0) == (g >= 2) and not dropped
    assert r.counts["dropped: " + ("stray class" if how == "stray class" else "assumed classes")] == 1


@pytest.mark.parametrize("mode", [1, 2])
def test_two_sets_taking_turns_never_adopt_each_others_noise(rule, mode):
    r = rule(mode)
    for g in range(6):
        for rows in (A, B):
            took, _, _ = r.multi_step(rows, 0.02, 3)
            assert took == -1
    for g in range(6):
        for rows in (A, B):
            took, _ = r.text_step(rows, 0.05)
            assert took == -1
    assert r.counts["refused: rows"] >= 20
    # ... nor a set of the same first row and another width
    r.text_step(A, 0.05)
    assert r.forward((0, 2), 0.05) == -1 and r.counts["refused: rows"] >= 21


@pytest.mark.parametrize("mode", [1, 2])
def test_what_does_not_fit_is_not_adopted_and_dropped(rule, mode):
    r = rule(mode)
    r.multi_step(A, 0.02, 3)
    r.multi_step(A, 0.02, 3)
    assert "1" in r.state["pending"]
    assert r.forward(A, 0.05) == -1 and r.state["pending"] == "00"           # another level
    assert r.counts["refused: level"] == 1
    r.text_step(A, 0.05)
    r.write()                                                                # a host write between offer and pass
    assert r.forward(A, 0.05) == -1
    r.offer(A, 0.05)
    assert r.forward(A, 0.05, bottom=1) == -1 and r.counts["refused: bottom"] == 1
    r.offer(A, 0.05)
    assert r.forward(A, 0.0) == -1 and r.state["pending"] != "00"            # a pass without noise draws nothing
    assert r.forward(A, 0.05) >= 0
    r.offer(A, 0.05)
    r.free()
    assert r.forward(A, 0.05) == -1


def test_a_host_write_where_the_assumed_loss_would_have_been(rule):
    """the slot filled two ahead is stamped with a PREDICTED count, one pass and one loss on; an upload
    of a generator instead of the loss gives a different history of the same length"""
    r = rule(2)
    r.multi_step(A, 0.02, 3)
    took, launches, _ = r.multi_step(A, 0.02, 3)
    assert took >= 0 and len(launches) == 2 and r.state["pending"] == "11"
    two_ahead = launches[1]
    assert r.forward(A, 0.02) >= 0                      # the pass in between adopts the first
    assert r.state["pending"] != "00"
    r.write()                                           # ... and where its loss would have been
    assert r.state["moves"] == two_ahead[4]             # the count alone would have let it through
    assert r.state["pending"] == "00" and r.forward(A, 0.02) == -1
