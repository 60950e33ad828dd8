"""The catalogue of SETTLEMENT scripts: several library calls in a row on one of the exact nets of exact_cases.py, observed
ONCE, at the end.  numpy only; the oracle's driver loads oracle/liboracle.so when it is made, the device's driver lives in
tests/test_gpu_settle.py.

The engine puts work off between calls and lets whichever call needs the result settle it:
  * the split-K planes of ih_delta and ho_delta that rnn_amd_set_calc_deltas(accumulate 0) leaves unsummed -- added up by
    k_apply on the update's way, by k_delta_finalize when somebody wants the arrays, or in front of an accumulating call;
    dropped by a second non-accumulating call, a clear, a per-net call that does not accumulate;
  * a lazy rnn_bptt_clear_deltas -- absorbed by the next accumulating call (which then does not accumulate) or carried out;
  * the error images of the last delta call's rows -- flushed, or handed to a ranged call on the same rows;
  * which of the host's and the device's copies is the valid one, per array class and per stream.
tests/test_gpu_exact_generations.py observes every step with a snapshot that begins by syncing everything, so every one
of these is settled there by the same route every time.  Here nothing looks in between: a script is a producer, what
comes between, `update` and `forward`, and one snapshot.  On the exact nets no order of summation rounds, so the one
snapshot owes the reference every element exactly, whoever settled what.

A script is a list of operations (`Script.ops`), each with the bits rnn_amd_set_deferred must show after it on the device:
  ("delta", k, acc)        generation G0 + k: advance, opinion, put_o_error, rnn_amd_set_calc_deltas(acc) with the case's
                           ranges and mask
  ("delta_one", k, j, acc) the same generation, the delta call for stream j alone through the per-net rnn_bptt_calc_deltas
                           on nets[j] (its o_error row written on the host, as that call's callers do); restated as
                           calc_deltas with a one-stream mask
  ("clear",)               rnn_bptt_clear_deltas
  ("sync", what, j)        rnn_amd_sync_host of ONE class (what: "WEIGHTS", "MOMENTUMS", "DELTAS", "STREAM"; j: the stream)
  ("edit_deltas",)         sync DELTAS, add 2^-10 to ih_delta[EDIT_IH] and ho_delta[EDIT_HO] on the host, host_written DELTAS
  ("regrow",)              three forward-only rnn_clones of the prototype (Fcap 1 -> 3, the regrow of test_gpu_dist.py) and
                           one rnn_opinion on the last, which is the call that finds the image too small and grows it right
                           there; a fixed seed, so that no generator moves; deleted at the end
  ("update",)              rnn_apply_learning with the script's method
  ("forward", k)           advance, opinion of generation G0 + k
In front of every script D forward passes fill the ring (`warm_up`): G0 = D, and g0, g1 of the tables are k = 0, 1.

The bits are written as letters: P the case's planes (ih and ho planes for ragged, h256, h512; the ih planes alone under
error ranges, whose top delta is summed at once; "masked" is the ragged net under an active mask), C a pending clear, E pending error images.  With RECUR_AMD_KEEP_DELTAS=0
the engine keeps no planes: P is then nothing, and everything else is as written.

`wrong` names, per script, the wrong settlements it is there to catch; RestatedDriver carries them out
(tests/test_settle_cases_cpu.py shows that each changes the final snapshot)."""
import numpy as np

import exact_cases as ec

IH_PLANES, HO_PLANES, CLEAR, IMAGES, TOP_DONE = 1, 2, 4, 8, 16
EDIT = 2.0 ** -10
EDIT_IH = (0, 1)    # the bias row of hidden unit 1
EDIT_HO = (1, 0)    # hidden unit 1 to output 0
STREAM_J = 2        # the stream of the per-net calls and of the one-stream sync
METHODS = {"WEIGHTED": ec.WEIGHTED, "NESTEROV": ec.NESTEROV, "CLASSICAL": ec.CLASSICAL}

# The cases: four of exact_cases.py's as they are, and "masked": the ragged net under the walking active mask of "ranged",
# without ranges -- a stream that the second of two set calls leaves out keeps BOTH its error images as the first left them
CASES = dict({k: ec.CASES[k] for k in ("ragged", "h256", "h512", "ranged")},
             masked=dict(ec.CASES["ragged"], masked=True,
                         forms=dict(ec.CASES["ragged"]["forms"], calc_args=dict(dense_inputs=1, active=1))))
# the planes each case's producer leaves (tests/test_settle_cases_cpu.py asks calc_plan.h)
PLANES = {"ragged": IH_PLANES | HO_PLANES, "h256": IH_PLANES | HO_PLANES, "h512": IH_PLANES | HO_PLANES, "ranged": IH_PLANES,
          "masked": IH_PLANES | HO_PLANES}

WRONG = ("planes_never_added", "planes_added_twice", "clear_lost", "overwrite_is_an_add", "edit_lost", "edit_on_stale_arrays",
         "images_zeroed")


def bits(case_name, letters, keep=True):
    """the letters of a script as rnn_amd_set_deferred's bits for a case; keep: the engine keeps planes"""
    return ((PLANES[case_name] if keep and "P" in letters else 0) | (CLEAR if "C" in letters else 0) |
            (IMAGES if "E" in letters else 0))


class Script:
    def __init__(self, name, ops, wrong, held, method=None):
        """ops: [(operation, letters after it)]; every script ends update, forward; method: None for the case's own"""
        self.name, self.wrong, self.held, self.method = name, wrong, held, method
        self.ops = [(op, letters) for op, letters in ops] + [(("forward", 2), None)]
        assert self.ops[-2][0] == ("update",) and set(wrong) <= set(WRONG)
        assert len({op[1] for op, _ in self.ops if op[0] in ("delta", "delta_one")}) <= 2    # two generations at the most

    def case(self, case_name):
        c = CASES[case_name]
        return c if self.method is None else dict(c, method=METHODS[self.method])


J = STREAM_J
_D0, _D1 = ("delta", 0, 0), ("delta", 0, 1)
# (a per-net delta call flushes the images and hands its own back: E is gone behind it;  a regrow evicts every stream)
PLANE_SCRIPTS = [
    Script("apply_takes_planes[%s]" % m, [(_D0, "PE"), (("update",), "E")], ("planes_never_added", "planes_added_twice"),
           "k_apply sums the planes on the update's way (rule %d)" % (1 if m == "NESTEROV" else 0), method=m)
    for m in METHODS
] + [
    Script("sync_takes_planes", [(_D0, "PE"), (("sync", "DELTAS", 0), "E"), (("update",), "E")],
           ("planes_added_twice", "planes_never_added"), "k_delta_finalize sums them, the update reads plain deltas"),
    Script("accumulate_on_planes", [(_D0, "PE"), (("delta", 1, 1), "E"), (("update",), "E")],
           ("planes_never_added", "planes_added_twice"), "materialise, then add"),
    Script("overwrite_planes", [(_D0, "PE"), (("delta", 1, 0), "PE"), (("update",), "E")],
           ("overwrite_is_an_add",), "g0's sums are gone"),
    Script("clear_drops_planes", [(_D0, "PE"), (("clear",), "CE"), (("update",), "E")],
           ("clear_lost",), "the weights move by momentum alone, the deltas read back as zeros"),
    Script("per_net_on_planes", [(_D0, "PE"), (("delta_one", 1, J, 1), ""), (("update",), "")],
           ("planes_never_added", "planes_added_twice"), "a per-net accumulating call on kept planes"),
    Script("per_net_drops_planes", [(_D0, "PE"), (("delta_one", 1, J, 0), ""), (("update",), "")],
           ("overwrite_is_an_add",), "a per-net non-accumulating call on kept planes"),
    # (the call that absorbs the clear does not accumulate -- and so leaves planes of its own)
    Script("clear_then_accumulate", [(_D1, "E"), (("clear",), "CE"), (("delta", 1, 1), "PE"), (("update",), "E")],
           ("clear_lost",), "the lazy clear absorbed by a set call"),
    Script("clear_then_accumulate_one", [(_D1, "E"), (("clear",), "CE"), (("delta_one", 1, J, 1), ""), (("update",), "")],
           ("clear_lost",), "the lazy clear absorbed by a per-net call"),
    Script("clear_then_sync", [(_D1, "E"), (("clear",), "CE"), (("sync", "DELTAS", 0), "E"), (("delta", 1, 1), "E"),
                               (("update",), "E")], ("clear_lost",), "the lazy clear carried out"),
    Script("edit_on_planes", [(_D0, "PE"), (("edit_deltas",), "E"), (("update",), "E")],
           ("edit_lost", "edit_on_stale_arrays", "planes_added_twice"), "a host edit on top of kept planes"),
    Script("regrow_on_planes", [(_D0, "PE"), (("regrow",), ""), (("update",), "")],
           ("planes_never_added", "planes_added_twice"), "a device regrow while planes are kept"),
    Script("regrow_on_clear", [(_D1, "E"), (("clear",), "CE"), (("regrow",), ""), (("delta", 1, 1), "E"), (("update",), "E")],
           ("clear_lost",), "a device regrow while a clear is pending"),
    Script("weights_only_sync", [(_D0, "PE"), (("sync", "WEIGHTS", 0), "PE"), (("sync", "MOMENTUMS", 0), "PE"), (("update",), "E")],
           ("planes_never_added", "planes_added_twice"), "a sync that must not settle the planes, nor disturb them"),
]
RANGED_SCRIPTS = [
    Script("ranged_twice", [(_D0, "PE"), (("delta", 1, 1), "E"), (("update",), "E")],
           ("images_zeroed", "planes_never_added"), "the same rows again: the images handed on as pending"),
    Script("ranged_then_one", [(_D0, "PE"), (("delta_one", 1, J, 1), ""), (("update",), "")],
           ("images_zeroed", "planes_never_added"), "flushed, then h_error written from the host"),
    Script("ranged_then_stream_sync", [(_D0, "PE"), (("sync", "STREAM", J), "P"), (("delta", 1, 1), "E"), (("update",), "E")],
           ("images_zeroed", "planes_never_added"), "flushed by one stream's sync, then the ranged call on every row"),
]
MASKED_SCRIPTS = [
    Script("masked_twice", [(_D0, "PE"), (("delta", 1, 1), "E"), (("update",), "E")],
           ("images_zeroed", "planes_never_added"), "a stream left out of the second call keeps the first call's images"),
]
SCRIPTS = {"ragged": PLANE_SCRIPTS, "h256": PLANE_SCRIPTS, "h512": PLANE_SCRIPTS, "ranged": RANGED_SCRIPTS,
           "masked": MASKED_SCRIPTS}
PAIRS = [(name, s.name) for name, scripts in SCRIPTS.items() for s in scripts]
# which scripts the oracle itself runs (tests/test_settle_cases_cpu.py): all of them on the small nets, two on the larger
# ones, whose other scripts are the same restated operations on other numbers
ON_THE_ORACLE = [(n, s) for n, s in PAIRS if n in ("ragged", "ranged", "masked") or s.startswith("apply_takes_planes") or s == "accumulate_on_planes"]


def script(case_name, script_name):
    return next(s for s in SCRIPTS[case_name] if s.name == script_name)


def warm_up(c):
    """the forward passes in front of every script: every ring slot is written once"""
    return [("forward", k - c["D"]) for k in range(c["D"])]


def one_stream(c, j):
    a = np.zeros(c["S"], np.uint8)
    a[j] = 1
    return a


def carry_out(driver, c, s):
    """the warm-up and the script on a driver; -> the driver"""
    for op in warm_up(c):
        getattr(driver, op[0])(*op[1:])
    for op, letters in s.ops:
        getattr(driver, op[0])(*op[1:])
        driver.after(op, letters)
    return driver


class RestatedDriver:
    """a script on exact_cases.Restated; wrong: one of WRONG, the settlement to get wrong"""

    def __init__(self, c, wrong=None, budget=None):
        self.c, self.wrong = c, wrong
        self.net = ec.net_of(c)
        self.r = ec.Restated(c, self.net, budget=budget)
        self.G0 = c["D"]
        self.stale = None       # the delta arrays in front of the producer
        self.deltas = 0         # delta calls so far

    def after(self, op, letters):
        pass

    def _forward(self, g, stage="hidden"):
        self.r.advance()
        self.r.opinion(ec.inputs_of(self.c, g), stage)

    def _calc(self, g, acc, active):
        c, r = self.c, self.r
        self._forward(g)
        r.o_error = ec.error_rows(c, g, self.net["zero_cols"]).astype(np.float64)
        if self.deltas == 0:
            self.stale = (r.ih_delta.copy(), r.ho_delta.copy())
        elif self.wrong == "overwrite_is_an_add":
            acc = 1
        elif self.wrong == "images_zeroed":
            r.err_a[:] = 0
        r.calc_deltas(acc, c["ranges"], active)
        if self.deltas == 0 and not acc:
            # the producer's sums are planes now: lost (the arrays stay what they were), or added up twice
            if self.wrong == "planes_never_added":
                r.ih_delta[:], r.ho_delta[:] = self.stale
            elif self.wrong == "planes_added_twice":
                r.ih_delta *= 2
                r.ho_delta *= 2
        self.deltas += 1

    def delta(self, k, acc):
        g = self.G0 + k
        self._calc(g, acc, ec.active_mask(self.c, g) if self.c["masked"] else None)

    def delta_one(self, k, j, acc):
        self._calc(self.G0 + k, acc, one_stream(self.c, j))

    def clear(self):
        if self.wrong != "clear_lost":
            self.r.clear_deltas()

    def sync(self, what, j):
        pass

    def regrow(self):
        pass

    def edit_deltas(self):
        r = self.r
        if self.wrong == "edit_lost":
            return
        if self.wrong == "edit_on_stale_arrays":
            r.ih_delta[:], r.ho_delta[:] = self.stale
        r.ih_delta[EDIT_IH] += EDIT
        r.ho_delta[EDIT_HO] += EDIT
        r.ih_abs[EDIT_IH] += EDIT
        r.ho_abs[EDIT_HO] += EDIT

    def update(self):
        self.r.apply_learning()
        self.updated = True

    def forward(self, k):
        self._forward(self.G0 + k, "hidden after" if getattr(self, "updated", False) else "hidden")

    def snapshot(self):
        return self.r.snapshot()


class OracleDriver:
    """a script on oracle/liboracle.so, through exact_cases.OracleSide"""

    def __init__(self, c):
        self.c = c
        self.side = ec.OracleSide(c)
        self.G0 = c["D"]

    def after(self, op, letters):
        pass

    def _calc(self, g, acc, active):
        c, side, o = self.c, self.side, self.side.o
        x, e = ec.fed(c, ec.inputs_of(c, g)), ec.error_rows(c, g, side.net["zero_cols"])
        a = o.arrays()
        for j in range(c["S"]):
            o.orc.orc_advance(o.z, j)
            side._opinion(j, x)
            a["o_error"][j] = e[j]
        ranges = None if side.ranges is None else side.rc.iptr(side.ranges)
        for j in np.nonzero(active)[0]:
            o.orc.orc_calc_deltas(o.z, int(j), acc, ranges)
            acc = 1

    def delta(self, k, acc):
        self._calc(self.G0 + k, acc, ec.active_mask(self.c, self.G0 + k))

    def delta_one(self, k, j, acc):
        self._calc(self.G0 + k, acc, one_stream(self.c, j))

    def clear(self):
        self.side.o.orc.orc_clear_deltas(self.side.o.z)

    def sync(self, what, j):
        pass

    def regrow(self):
        pass

    def edit_deltas(self):
        a = self.side.o.arrays()
        a["ih_delta"][EDIT_IH] += np.float32(EDIT)
        a["ho_delta"][EDIT_HO] += np.float32(EDIT)

    def update(self):
        self.side.update()

    def forward(self, k):
        self.side.forward(self.G0 + k)

    def snapshot(self):
        return self.side.snapshot()

    def close(self):
        self.side.close()


def restated(case_name, script_name, wrong=None, budget=None):
    """-> the RestatedDriver after the script"""
    s = script(case_name, script_name)
    c = s.case(case_name)
    return carry_out(RestatedDriver(c, wrong, budget), c, s)


def on_the_oracle(case_name, script_name):
    """-> the oracle's snapshot after the script"""
    s = script(case_name, script_name)
    c = s.case(case_name)
    d = carry_out(OracleDriver(c), c, s)
    snap = d.snapshot()
    d.close()
    return snap
