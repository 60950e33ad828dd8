"""Deferred device state against the reference BIT FOR BIT, whoever settles it (tests/settle_cases.py; the CPU half,
tests/test_settle_cases_cpu.py, shows that no sum of a script can round, that the oracle gives what the restatement gives,
and that each script would notice the wrong settlement it is there for).

tests/test_gpu_exact_generations.py takes a snapshot after every step, and a snapshot begins by syncing everything: kept
delta planes, a pending clear and pending error images are settled there by one route, every time.  Here a script of
several calls runs UNOBSERVED -- no snapshot, no statistics, no call of the library but the script's own and the read-only
rnn_amd_set_deferred -- and one snapshot at its end is held as that file holds its own: every element of every array with
np.array_equal, the output layer behind the update within exact_cases.rounded_output_bound and at the bar; generators,
ring positions and generation counters.  No tolerance is new here.

rnn_amd_set_deferred is read after every operation and must show the bits the script states (P the case's planes, C a
pending clear, E pending error images): if the engine stopped keeping planes, or settled them earlier than the script
means, the test fails instead of passing by the eager route.  One further test runs the "ragged" and "h512" tests in a child
process with RECUR_AMD_KEEP_DELTAS=0 (read once per process): there no planes bit may ever show, and every array is owed
all the same -- the eager and the deferred route owe the same bits.

MEASURED on the MI355X, first run (the 51 scripts in 2.6 s): every deferred bit as the scripts state it, after every call;
39 scripts equal on every array.  EQUAL on all three nets: apply_takes_planes (the three methods), sync_takes_planes,
clear_drops_planes, per_net_on_planes, per_net_drops_planes, clear_then_accumulate_one, edit_on_planes, regrow_on_planes,
regrow_on_clear, weights_only_sync; and the three ranged scripts.  NOT EQUAL, on all three nets: accumulate_on_planes,
overwrite_planes, clear_then_accumulate, clear_then_sync -- the four scripts with two SET delta calls in a row -- and in
err_a alone: 3 of 312 entries (ragged), 1 of 9344 (h256), 5 of 68096 (h512), each 0.0 where the reference has a small
dyadic number, each at a column from h_size on (47 of 52; 282 of 292; 517 of 532) of a stream whose second run executes
ONE step (the generation's all-zero error row among them).  The reference's one-step run writes h_error's first h_size
entries and leaves the rest as the run before left them (write_error_images, n == 1); between two set calls over the same
rows without ranges the engine skips k_err_writeback, because the second call's images replace the first's -- so the
entries the second run should have KEPT had never been written, and the device showed what was there before the first
run: stale images zeroed, the wrong settlement the ranged scripts were written for, found where there are no ranges.
Nothing computes with those entries; a caller who reads bptt->h_error sees them.  Fixed in bptt_control_wave (k_extras.h):
a run of two or more steps leaves h_error's entries from h_size on at once (one row's input columns from the extras plane
stale_plane(n); k_bptt_small writes its images itself), and in ramd_set_calc_deltas (set_api.c): a masked call that leaves a
stream out, whose images are to stay WHOLE, rebuilds the pending images first (masked_twice, the ragged net under the
walking mask, was added to the catalogue with it).  Second run: every script and the child equal.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_cases as ec
import recur_ctypes as rc
import settle_cases as st
import test_gpu_exact_generations as xg

pytestmark = pytest.mark.gpu
KEEP = not os.environ.get("RECUR_AMD_KEEP_DELTAS", "").startswith("0")     # (as set_api.c reads it)
WHAT = {"WEIGHTS": rc.RNN_AMD_WEIGHTS, "MOMENTUMS": rc.RNN_AMD_MOMENTUMS, "DELTAS": rc.RNN_AMD_DELTAS, "STREAM": rc.RNN_AMD_STREAM}
CLONE_SEED = 7     # (a seed of its own: rnn_clone draws nothing from the prototype's generator)


@pytest.fixture(scope="module")
def amd():
    lib = rc.load_amd()
    assert lib.rnn_amd_device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return lib


@functools.lru_cache(maxsize=None)
def reference(case_name, script_name):
    """-> (the Restated after the script, its snapshot), once per (case, script)"""
    d = st.restated(case_name, script_name)
    return d.r, d.snapshot()


class DeviceDriver(xg.DeviceSide):
    """a script on librecur_amd.so.  Between the written net and the final snapshot it makes the script's own calls and
    reads rnn_amd_set_deferred; nothing else."""

    def __init__(self, lib, case_name, c):
        super().__init__(lib, c)
        self.case_name, self.G0 = case_name, c["D"]
        self.clones, self.bad = [], []

    def after(self, op, letters):
        if letters is None:
            return
        got, want = self.lib.rnn_amd_set_deferred(self.g.handle), st.bits(self.case_name, letters, KEEP)
        if got != want:
            self.bad.append("deferred after %s: %d, the script says %d (%s)" % (op, got, want, letters))

    def _put(self, g):
        e = np.ascontiguousarray(ec.error_rows(self.c, g, self.net["zero_cols"]))
        self._advance()
        self._opinion(ec.inputs_of(self.c, g))
        self.lib.rnn_amd_set_put_o_error(self.g.handle, rc.fptr(e), e.shape[1])
        return e

    def delta(self, k, acc):
        g = self.G0 + k
        self._put(g)
        act = np.ascontiguousarray(ec.active_mask(self.c, g))
        self.lib.rnn_amd_set_calc_deltas(self.g.handle, acc, self.ranges, rc.u8ptr(act) if self.c["masked"] else None)

    def delta_one(self, k, j, acc):
        e = self._put(self.G0 + k)
        net = self.g.nets[j]
        rc.view(net.contents.bptt.contents.o_error, self.g.O)[:] = e[j]    # (the per-net call takes the host's row)
        self.lib.rnn_bptt_calc_deltas(net, acc, self.ranges)

    def clear(self):
        self.lib.rnn_bptt_clear_deltas(self.g.net)

    def sync(self, what, j):
        self.lib.rnn_amd_sync_host(self.g.nets[j], WHAT[what])

    def edit_deltas(self):
        g, b0 = self.g, self.g.net.contents.bptt.contents
        self.lib.rnn_amd_sync_host(g.net, rc.RNN_AMD_DELTAS)
        rc.view(b0.ih_delta, g.I, g.H)[st.EDIT_IH] += np.float32(st.EDIT)
        rc.view(b0.ho_delta, g.H, g.O)[st.EDIT_HO] += np.float32(st.EDIT)
        self.lib.rnn_amd_host_written(g.net, rc.RNN_AMD_DELTAS)

    def regrow(self):
        g = self.g
        fl = g.net.contents.flags & ~(rc.FLAG_OWN_WEIGHTS | rc.FLAG_OWN_BPTT)
        self.clones = [self.lib.rnn_clone(g.net, fl, CLONE_SEED, None) for _ in range(3)]     # Fcap 1 -> 3
        rc.view(self.clones[2].contents.real_inputs, g.input_size)[:] = 0
        self.lib.rnn_opinion(self.clones[2], None, 0.0)     # (the call that grows the image)

    def forward(self, k):
        super().forward(self.G0 + k)

    def close(self):
        for n in self.clones:
            self.lib.rnn_delete_net(n)
        super().close()


@pytest.mark.parametrize("case_name,script_name", st.PAIRS)
def test_every_array_behind_the_script_is_the_references(amd, case_name, script_name):
    s = st.script(case_name, script_name)
    c = s.case(case_name)
    r, want = reference(case_name, script_name)
    dev = DeviceDriver(amd, case_name, c)
    st.carry_out(dev, c, s)
    got = dev.snapshot()
    bad = dev.bad + xg.compare(got, want, r, True)
    if not np.array_equal(got["rng"], dev.start["rng"]):
        bad.append("rng: a generator has moved")
    dev.close()
    print("%s, %s (%s): %s" % (case_name, script_name, s.held, "every element equal" if not bad else "; ".join(bad)))
    assert not bad, "%s, %s: %s" % (case_name, script_name, " | ".join(bad))


def test_the_scripts_owe_the_same_bits_when_no_planes_are_kept():
    """RECUR_AMD_KEEP_DELTAS=0 is read once per process: one child runs the "ragged" and "h512" tests of this file with
    it.  There `P` is nothing -- a planes bit that shows fails the child's test -- and every array is still the
    reference's."""
    if not KEEP:
        return    # (this IS the child)
    e = dict(os.environ, RECUR_AMD_KEEP_DELTAS="0")
    n = len(st.SCRIPTS["ragged"]) + len(st.SCRIPTS["h512"])
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-p", "no:cacheprovider", "-m", "gpu",
                        "-k", "test_every_array and (ragged or h512)"],
                       capture_output=True, text=True, env=e, timeout=600, cwd=os.path.dirname(os.path.abspath(__file__)))
    assert r.returncode == 0 and "%d passed" % n in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
