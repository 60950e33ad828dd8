"""Rate probe: what the per-text states of the batched text calls cost.  Workload: gpu_texts_rate.py's -- 42 symbols, 256
texts of 400 - 600 symbols from tests/golden/erewhon.txt, at hidden 1024 and at hidden 99 -- scored three ways:

    (a) one rnn_amd_run_texts                                      (no states: what the call always was)
    (b) one rnn_amd_run_texts_from with h_in and h_out             (one copy of 256 x h_size floats each way)
    (c) the same texts in windows of 128 symbols, states in place  (rnn_amd_run_texts_from once per window: the windows
                                                                    overlap by one symbol, every symbol is fed once)

All forms are warmed up, timed by the host clock around work that ends in a device synchronisation, and alternated in the
same run; the figures are symbols per second (a symbol = one forward pass of one text), every round's seconds, and the
largest relative difference of (b)'s and (c)'s sums from (a)'s -- (b) starts every text from the net's own hidden row, so
its sums are (a)'s bit for bit; (c) runs its later windows at other row counts: the bar, not the bits.

Run from a checkout that does not have the _from calls (the parent of the commit that added them) it measures (a) alone:
profiles/r07_states_rate.txt holds both checkouts' (a) from alternating runs in one session.

    python tools/gpu_states_rate.py [rounds]          # writes what profiles/r07_states_rate.txt holds
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import recur_ctypes as rc  # noqa: E402
import scenarios as sc  # noqa: E402
from recur_amd import drivers  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
N_TEXTS, SYMBOLS, WINDOW = 256, 42, 128
WITH_STATES = hasattr(drivers, "run_texts_from")


def main():
    amd = rc.bind_char(rc.load_amd())
    if amd.rnn_amd_device_count() < 1:
        raise SystemExit("gpu_states_rate.py needs a HIP device: a rate is measured on the GPU or not at all")
    text = rc.encode_erewhon(amd)
    rng = np.random.default_rng(7)
    lens = rng.integers(400, 601, N_TEXTS)
    starts = rng.integers(30000, len(text) - 601, N_TEXTS)
    texts = [np.ascontiguousarray(text[a:a + n]) for a, n in zip(starts, lens)]
    symbols = int((lens - 1).sum())
    windows = [[t[at:at + WINDOW] for t in texts] for at in range(0, int(lens.max()) - 1, WINDOW - 1)]
    print("workload: %d texts of %d .. %d symbols (%d forward passes of one text in all), %d symbols in the alphabet; "
          "(c): %d windows of %d symbols; %s"
          % (N_TEXTS, lens.min(), lens.max(), symbols, SYMBOLS, len(windows), WINDOW,
             "all three forms" if WITH_STATES else "this checkout has no _from calls: (a) alone"))
    for hidden in (1024, 99):
        a = sc.AmdBatchedSet(amd, input_size=SYMBOLS, hidden_size=hidden, output_size=SYMBOLS, S=4, D=10, learn_rate=1e-3, seed=1)
        a.load_text(np.ascontiguousarray(text[:20000]))
        for i in range(40):  # weights that are not the initial ones
            amd.rnn_amd_set_char_step(a.handle, i, rc.WEIGHTED, 0.9)
        flags = a.net.contents.flags & ~(rc.FLAG_OWN_BPTT | rc.FLAG_OWN_WEIGHTS)
        scorer = amd.rnn_clone(a.net, flags, rc.SUBSEED, None)
        amd.rnn_amd_sync_host(scorer, rc.RNN_AMD_STREAM)
        own = np.tile(rc.view(scorer.contents.hidden_layer, a.H).copy(), (N_TEXTS, 1))  # every text from the net's own row

        def clocked(work):
            amd.rnn_amd_synchronize()
            t0 = time.perf_counter()
            sums = work()
            amd.rnn_amd_synchronize()
            return sums, time.perf_counter() - t0

        def plain():
            return drivers.run_texts(amd, scorer, texts)

        def with_states():
            return drivers.run_texts_from(amd, scorer, texts, h_in=own)[0]

        def windowed():
            states, total = own.copy(), np.zeros(N_TEXTS)
            for part in windows:
                total += drivers.run_texts_from(amd, scorer, part, h_in=states, in_place=True)[0]
            return total

        forms = [("(a) rnn_amd_run_texts", plain)]
        if WITH_STATES:
            forms += [("(b) rnn_amd_run_texts_from, both states", with_states), ("(c) windows of %d, states in place" % WINDOW, windowed)]
        for _, work in forms:  # warm-up: every kernel of every form has run at its shapes
            clocked(work)
        times = {name: [] for name, _ in forms}
        sums = {}
        for r in range(ROUNDS):
            for name, work in forms:
                sums[name], dt = clocked(work)
                times[name].append(dt)
        base = sums[forms[0][0]]
        for name, _ in forms:
            t = times[name]
            print("hidden %4d: %-42s %10.0f symbols/s, median %.4f s (%s); largest relative difference from (a)'s sums %.2e"
                  % (hidden, name, symbols / np.median(t), np.median(t), " ".join("%.4f" % x for x in t),
                     float(np.max(np.abs(sums[name] - base) / np.abs(base)))))
        if WITH_STATES:
            ta = np.median(times[forms[0][0]])
            print("hidden %4d: (b) / (a) = %.4f of the time, (c) / (a) = %.4f; states: %d x %d floats = %.2f MB each way"
                  % (hidden, np.median(times[forms[1][0]]) / ta, np.median(times[forms[2][0]]) / ta, N_TEXTS, a.H,
                     N_TEXTS * a.H * 4 / 1e6))
        amd.rnn_delete_net(scorer)
        a.close()


if __name__ == "__main__":
    main()
