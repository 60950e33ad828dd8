"""Rate probe: what it costs to run a trained text classifier over many texts and add up the class probabilities.  Three
routes, warmed up, alternated in the same process and timed by the host clock around work that ends in a device
synchronisation -- the caller's arrays made before the clock starts:

  (a) today's loop, text-classify-results' (text-classify-results.c:83-122): per text a fresh forward-only clone, per symbol
      one rnn_opinion of the one-hot row -- which synchronises and copies the output row to the host -- then the host's
      softmax (the oracle's, compiled C) and sum += a, sumsq += a * a in numpy float64.  A per-symbol loop costs the same
      for every symbol, so it runs over the first LOOP_TEXTS texts only and its rate is symbols of those per second.
  (b) today's batched route: the texts expanded on the host into dense one-hot rows (outside the clock), one
      rnn_amd_run_sequences with all outputs as one class group, and its answers summed on the host in float64 (inside the
      clock: the sums are what is wanted).
  (c) the new call: one rnn_amd_classify_texts with sums and sums of squares, and -- (c') -- the same with a class byte
      per symbol and the scores.

The loops are driven from Python through ctypes, as every probe here is; clones are made and deleted outside the clock.
Workload: 256 texts of 400 - 600 symbols of 42, 8 classes, at hidden 99 and at hidden 1024, seeded weights.  Figures are
symbols per second (a symbol = one forward pass of one text).

    python tools/gpu_classify_rate.py [rounds]          # writes what profiles/r12_classify_texts_rate.txt holds
"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import recur_ctypes as rc  # noqa: E402
from recur_amd.drivers import TRACE_GUARD  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
N_TEXTS, SYMBOLS, CLASSES, LOOP_TEXTS = 256, 42, 8, 32


def main():
    amd = rc.load_amd()
    if amd.rnn_amd_device_count() < 1:
        raise SystemExit("gpu_classify_rate.py needs a HIP device: a rate is measured on the GPU or not at all")
    orc = rc.load_oracle()
    rng = np.random.default_rng(7)
    lens = rng.integers(400, 601, N_TEXTS).astype(np.int32)
    texts = [rng.integers(0, SYMBOLS, n).astype(np.uint8) for n in lens]
    classes = [rng.integers(0, CLASSES, n).astype(np.uint8) for n in lens]
    total = int(lens.sum())
    looped = int(lens[:LOOP_TEXTS].sum())
    print("workload: %d texts of %d .. %d symbols of %d (%d forward passes of one text in all), %d classes; (a) runs the "
          "first %d texts, %d symbols" % (N_TEXTS, lens.min(), lens.max(), SYMBOLS, total, CLASSES, LOOP_TEXTS, looped))
    print("(b) uploads %d bytes a symbol and downloads %d; (c) uploads 1 (with classes 2) and downloads %d a text"
          % (4 * SYMBOLS, 4 * CLASSES, 8 * (2 * CLASSES + 4)))
    eye = np.eye(SYMBOLS, dtype=np.float32)
    seqs = [np.ascontiguousarray(eye[t]) for t in texts]   # (b)'s dense rows: made outside the clock
    inp = (rc.c_float_p * N_TEXTS)(*[rc.fptr(s) for s in seqs])
    tp = (rc.c_u8_p * N_TEXTS)(*[rc.u8ptr(t) for t in texts])
    cp = (rc.c_u8_p * N_TEXTS)(*[rc.u8ptr(c) for c in classes])
    goff, gsize = np.array([0], np.int32), np.array([CLASSES], np.int32)
    dp = C.POINTER(C.c_double)
    for hidden in (99, 1024):
        net = amd.rnn_new(SYMBOLS, hidden, CLASSES, rc.FLAG_STANDARD, 11, None, 4, 1e-3, 0.9, 0.0, rc.RELU)
        amd.rnn_randomise_weights_auto(net)
        flags = net.contents.flags & ~(rc.FLAG_OWN_BPTT | rc.FLAG_OWN_WEIGHTS)
        p = np.zeros(CLASSES, np.float32)
        pp = rc.fptr(p)

        def loop(which):
            """(a): per symbol rnn_opinion of the one-hot row, the host's softmax, the sums"""
            clones = [amd.rnn_clone(net, flags, rc.SUBSEED, None) for _ in which]
            last = amd.rnn_clone(net, flags, rc.SUBSEED, None)
            amd.rnn_opinion(last, rc.fptr(eye[0]), 0.0)  # (the device image grows for the clones here)
            amd.rnn_amd_synchronize()
            sums, sumsqs = np.zeros((len(which), CLASSES)), np.zeros((len(which), CLASSES))
            t0 = time.perf_counter()
            for c, k, s, q in zip(clones, which, sums, sumsqs):
                real = rc.view(c.contents.real_inputs, SYMBOLS)
                real[:] = 0.0
                hot = 0
                for symbol in texts[k]:
                    real[hot] = 0.0
                    hot = int(symbol)
                    real[hot] = 1.0
                    ans = amd.rnn_opinion(c, None, 0.0)
                    orc.orc_softmax(pp, ans, CLASSES)
                    s += p
                    q += p * p
            amd.rnn_amd_synchronize()
            dt = time.perf_counter() - t0
            for c in [last] + clones[::-1]:
                amd.rnn_delete_net(c)
            return sums, sumsqs, dt

        def dense():
            """(b): one rnn_amd_run_sequences over the one-hot rows, the answers summed on the host"""
            ans = [np.full(n * CLASSES + TRACE_GUARD, np.nan, np.float32) for n in lens]
            ansp = (rc.c_float_p * N_TEXTS)(*[rc.fptr(x) for x in ans])
            amd.rnn_amd_synchronize()
            t0 = time.perf_counter()
            r = amd.rnn_amd_run_sequences(scorer, inp, rc.iptr(lens), N_TEXTS, SYMBOLS, 1, rc.iptr(goff), rc.iptr(gsize),
                                          None, None, 0, ansp, None)
            rows = [x[:n * CLASSES].reshape(-1, CLASSES) for x, n in zip(ans, lens)]
            sums = np.stack([x.sum(axis=0, dtype=np.float64) for x in rows])
            sumsqs = np.stack([(x * x).sum(axis=0, dtype=np.float64) for x in rows])
            amd.rnn_amd_synchronize()
            dt = time.perf_counter() - t0
            assert r == 0
            return sums, sumsqs, dt

        def batched(scored):
            """(c): one rnn_amd_classify_texts; the arrays are the caller's and are made outside the clock"""
            sums, sumsqs = np.full((N_TEXTS, CLASSES), np.nan), np.full((N_TEXTS, CLASSES), np.nan)
            scores = (rc.ClassScore * N_TEXTS)()
            amd.rnn_amd_synchronize()
            t0 = time.perf_counter()
            r = amd.rnn_amd_classify_texts(scorer, tp, rc.iptr(lens), None, cp if scored else None, N_TEXTS, None, None,
                                           sums.ctypes.data_as(dp), sumsqs.ctypes.data_as(dp), scores if scored else None)
            amd.rnn_amd_synchronize()
            dt = time.perf_counter() - t0
            assert r == 0 and (not scored or sum(s.count for s in scores) == total)
            return sums, sumsqs, dt

        scorer = amd.rnn_clone(net, flags, rc.SUBSEED, None)  # hidden row zero, like the loop's fresh clones
        loop(list(range(2)))  # warm-up: every kernel of the three routes has run at its shapes
        dense()
        batched(False)
        batched(True)
        t_a, t_b, t_c, t_d = [], [], [], []
        for r in range(ROUNDS):
            s_a, q_a, dt = loop(list(range(LOOP_TEXTS)))
            t_a.append(dt)
            s_b, q_b, dt = dense()
            t_b.append(dt)
            s_c, q_c, dt = batched(False)
            t_c.append(dt)
            s_d, q_d, dt = batched(True)
            t_d.append(dt)
            assert np.array_equal(s_c, s_d) and np.array_equal(q_c, q_d)
        ra, rb = looped / np.median(t_a), total / np.median(t_b)
        rc_, rd = total / np.median(t_c), total / np.median(t_d)
        print("hidden %4d: (a) loop of rnn_opinion + host softmax          %9.0f symbols/s (%s s for %d symbols)"
              % (hidden, ra, " ".join("%.3f" % t for t in t_a), looped))
        print("hidden %4d: (b) one-hot rows through rnn_amd_run_sequences  %9.0f symbols/s (%s s)"
              % (hidden, rb, " ".join("%.4f" % t for t in t_b)))
        print("hidden %4d: (c) one rnn_amd_classify_texts                  %9.0f symbols/s (%s s)"
              % (hidden, rc_, " ".join("%.4f" % t for t in t_c)))
        print("hidden %4d: (c') the same with classes and scores           %9.0f symbols/s (%s s)"
              % (hidden, rd, " ".join("%.4f" % t for t in t_d)))
        fastest = max((ra, "(a)"), (rb, "(b)"), (rc_, "(c)"))[1]
        print("hidden %4d: (c) / (a) = %.1f; (c) / (b) = %.2f; (c') / (c) = %.3f; the fastest of (a), (b), (c) is %s"
              % (hidden, rc_ / ra, rc_ / rb, rd / rc_, fastest))
        print("hidden %4d: (c) against (a): largest relative difference of a sum %.2e, of a sum of squares %.2e; against (b): "
              "%.2e, %.2e" % (hidden, float(np.abs(s_c[:LOOP_TEXTS] / s_a - 1).max()), float(np.abs(q_c[:LOOP_TEXTS] / q_a - 1).max()),
                              float(np.abs(s_c / s_b - 1).max()), float(np.abs(q_c / q_b - 1).max())))
        amd.rnn_delete_net(scorer)
        amd.rnn_delete_net(net)


if __name__ == "__main__":
    main()
