"""Rate probe: what it costs to know, symbol by symbol, how surprised a net was by many texts.  Three forms, warmed up,
alternated in the same run and timed by the host clock around work that ends in a device synchronisation -- for (b) and
(c) around the library call alone, the caller's arrays made before it:

  (a) the loop a caller writes today, colourise_text's (text-cross-entropy.c:91-116): per text a fresh forward-only clone,
      per symbol one rnn_opinion on the one-hot input -- which synchronises and copies the output row to the host -- then
      the softmax and the best guess on the host (the oracle's orc_softmax_best_guess, compiled C) and capped_log2f of
      the next symbol's likelihood.  The loop is driven from Python through ctypes, as every probe here is; the clones
      are made and deleted outside the clock.
  (b) one rnn_amd_run_texts: the sums alone.
  (c) one rnn_amd_trace_texts with guesses: every float of (b)'s sums and the best guess next to it.

(c) against (a) is what the trace replaces; (c) against (b), of the same run, is the price of the trace over the sums:
one more copy per wave -- 5 bytes per traced value -- and a few stores per row and step.  Workload: 42 symbols, 256
texts of 400 - 600 symbols from tests/golden/erewhon.txt, at hidden 1024 and at hidden 99.  Figures are symbols per
second (a symbol = one forward pass of one text); the three forms' figures are compared with each other in the output.

    python tools/gpu_trace_rate.py [rounds]          # writes what profiles/r07_trace_rate.txt holds
"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import recur_ctypes as rc  # noqa: E402
import scenarios as sc  # noqa: E402
from recur_amd.drivers import TRACE_GUARD, text_pointers  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
N_TEXTS, SYMBOLS = 256, 42


def main():
    amd = rc.bind_char(rc.load_amd())
    if amd.rnn_amd_device_count() < 1:
        raise SystemExit("gpu_trace_rate.py needs a HIP device: a rate is measured on the GPU or not at all")
    orc = rc.load_oracle()
    text = rc.encode_erewhon(amd)
    rng = np.random.default_rng(7)
    lens = rng.integers(400, 601, N_TEXTS)
    starts = rng.integers(30000, len(text) - 601, N_TEXTS)
    texts = [np.ascontiguousarray(text[a:a + n]) for a, n in zip(starts, lens)]
    symbols = int((lens - 1).sum())
    keep, ptrs, ln = text_pointers(texts)
    print("workload: %d texts of %d .. %d symbols (%d forward passes of one text in all), %d symbols in the alphabet"
          % (N_TEXTS, lens.min(), lens.max(), symbols, SYMBOLS))
    print("the trace of one call: %d values, %d bytes on the device and through one copy per wave" % (symbols, 5 * symbols))
    for hidden in (1024, 99):
        a = sc.AmdBatchedSet(amd, input_size=SYMBOLS, hidden_size=hidden, output_size=SYMBOLS, S=4, D=10, learn_rate=1e-3, seed=1)
        a.load_text(np.ascontiguousarray(text[:20000]))
        for i in range(40):  # weights that are not the initial ones
            amd.rnn_amd_set_char_step(a.handle, i, rc.WEIGHTED, 0.9)
        flags = a.net.contents.flags & ~(rc.FLAG_OWN_BPTT | rc.FLAG_OWN_WEIGHTS)
        err = np.zeros(SYMBOLS, np.float32)
        errp = rc.fptr(err)

        def loop(which):
            """(a): per symbol rnn_opinion, the host's softmax, capped_log2f"""
            clones = [amd.rnn_clone(a.net, flags, rc.SUBSEED, None) for _ in which]
            last = amd.rnn_clone(a.net, flags, rc.SUBSEED, None)
            amd.rnn_amd_run_text(last, rc.u8ptr(texts[0]), 2, 0)  # (the device image grows for the clones here)
            amd.rnn_amd_synchronize()
            logp = [np.zeros(len(texts[k]) - 1, np.float32) for k in which]
            guess = [np.zeros(len(texts[k]) - 1, np.uint8) for k in which]
            t0 = time.perf_counter()
            for c, k, lp, gs in zip(clones, which, logp, guess):
                t = [int(x) for x in texts[k]]
                real = rc.view(c.contents.real_inputs, SYMBOLS)
                for i in range(len(t) - 1):
                    real[t[i - 1] if i else 0] = 0.0
                    real[t[i]] = 1.0
                    ans = amd.rnn_opinion(c, None, 0.0)
                    gs[i] = orc.orc_softmax_best_guess(errp, ans, SYMBOLS)  # (leaves -softmax in err)
                    lp[i] = orc.orc_capped_log2f(-err[t[i + 1]])
            amd.rnn_amd_synchronize()
            dt = time.perf_counter() - t0
            for c in [last] + clones[::-1]:
                amd.rnn_delete_net(c)
            return logp, guess, dt

        def sums_only():
            sums = np.full(N_TEXTS, np.nan)
            amd.rnn_amd_synchronize()
            t0 = time.perf_counter()
            r = amd.rnn_amd_run_texts(scorer, ptrs, rc.iptr(ln), None, N_TEXTS, sums.ctypes.data_as(C.POINTER(C.c_double)))
            amd.rnn_amd_synchronize()
            dt = time.perf_counter() - t0
            assert r == 0
            return sums, dt

        def traced():
            """the arrays are the caller's and are made outside the clock, with guard entries behind them"""
            lp = [np.full(n - 1 + TRACE_GUARD, np.nan, np.float32) for n in lens]
            gs = [np.full(n - 1 + TRACE_GUARD, 0xEE, np.uint8) for n in lens]
            lpp = (rc.c_float_p * N_TEXTS)(*[rc.fptr(x) for x in lp])
            gsp = (rc.c_u8_p * N_TEXTS)(*[rc.u8ptr(x) for x in gs])
            amd.rnn_amd_synchronize()
            t0 = time.perf_counter()
            r = amd.rnn_amd_trace_texts(scorer, ptrs, rc.iptr(ln), N_TEXTS, 0, lpp, gsp)
            amd.rnn_amd_synchronize()
            dt = time.perf_counter() - t0
            assert r == 0
            assert all(np.all(np.isnan(x[n - 1:])) and np.all(y[n - 1:] == 0xEE) for x, y, n in zip(lp, gs, lens))
            return [(x[:n - 1].reshape(-1, 1), y[:n - 1].reshape(-1, 1)) for x, y, n in zip(lp, gs, lens)], dt

        scorer = amd.rnn_clone(a.net, flags, rc.SUBSEED, None)  # hidden row zero, like the loop's fresh clones
        loop(list(range(4)))  # warm-up: every kernel of the three forms has run at its shapes
        sums_only()
        traced()
        everything = list(range(N_TEXTS))
        t_a, t_b, t_c = [], [], []
        for r in range(ROUNDS):
            lp_a, gs_a, dt = loop(everything)
            t_a.append(dt)
            sums, dt = sums_only()
            t_b.append(dt)
            got, dt = traced()
            t_c.append(dt)
        ra, rb, rc_ = (symbols / np.median(t) for t in (t_a, t_b, t_c))
        flat_a, flat_c = np.concatenate(lp_a), np.concatenate([lp[:, 0] for lp, _ in got])
        same_guess = float(np.mean(np.concatenate(gs_a) == np.concatenate([gs[:, 0] for _, gs in got])))
        of_sums = all(float(np.cumsum(lp[:, 0].astype(np.float64))[-1]) == s for (lp, _), s in zip(got, sums))
        print("hidden %4d: (a) loop of rnn_opinion + host softmax %8.0f symbols/s (%s s)" % (hidden, ra, " ".join("%.3f" % t for t in t_a)))
        print("hidden %4d: (b) one rnn_amd_run_texts             %8.0f symbols/s (%s s)" % (hidden, rb, " ".join("%.4f" % t for t in t_b)))
        print("hidden %4d: (c) one rnn_amd_trace_texts, guesses  %8.0f symbols/s (%s s)" % (hidden, rc_, " ".join("%.4f" % t for t in t_c)))
        print("hidden %4d: (c) / (a) = %.1f; (c) / (b) = %.3f, the trace costs %.1f %% of the sums' time, %.2f ms a call"
              % (hidden, rc_ / ra, rc_ / rb, 100.0 * (np.median(t_c) / np.median(t_b) - 1.0), 1e3 * (np.median(t_c) - np.median(t_b))))
        print("hidden %4d: (c) against (a): largest |difference| of a log2 p %.2e (of %.2f .. %.2f), %.4f of the guesses the same; "
              "(c)'s floats add up to (b)'s sums bit for bit: %s; mean entropy %.3f bits"
              % (hidden, float(np.abs(flat_a - flat_c).max()), float(flat_c.min()), float(flat_c.max()), same_guess, of_sums,
                 float(-flat_c.sum() / symbols)))
        amd.rnn_delete_net(scorer)
        a.close()


if __name__ == "__main__":
    main()
