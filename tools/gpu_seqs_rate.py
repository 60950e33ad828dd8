"""Rate probe: what it costs to run a trained classifier over many recordings' features.  Three forms, warmed up,
alternated in the same run and timed by the host clock around work that ends in a device synchronisation -- the caller's
arrays made before the clock starts:

  (a) the loop a caller writes with the drop-in API, emit_opinions' (gstclassify.c:2259-2292): per recording a fresh
      forward-only clone, per frame one rnn_opinion on the frame's features -- which synchronises and copies the output
      row to the host -- then softmax_best_guess of the class group on the host (the oracle's, compiled C).
  (b) the loop a caller writes with the batched API: 256 forward-only clones as one set, per frame one
      rnn_amd_set_opinion over all of them -- one upload of 256 feature rows, one pass, one copy back of the answers,
      one synchronisation -- then the host's softmax_best_guess per recording that still runs.  The recordings are ragged,
      so the set computes rows that nobody wants (zeros are fed to a recording that has ended); only real frames count.
  (c) one rnn_amd_run_sequences with winners: at the default segment (64 frames at 32 features: up to ten segments per
      wave here) and at segments of 512 and 8 frames.

The loops are driven from Python through ctypes, as every probe here is; clones and sets are made and deleted outside the
clock.  Workload: 256 recordings of 400 - 600 frames of 32 features, 2 classes in one group, at hidden 512 and at hidden
1024, seeded weights.  Figures are frames per second (a frame = one forward pass of one recording).

    python tools/gpu_seqs_rate.py [rounds]          # writes what profiles/r07_seqs_rate.txt holds
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import recur_ctypes as rc  # noqa: E402
from recur_amd.drivers import TRACE_GUARD  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
N_SEQS, FEATURES, CLASSES = 256, 32, 2
SEGMENTS = [0, 512, 8]


def main():
    amd = rc.load_amd()
    if amd.rnn_amd_device_count() < 1:
        raise SystemExit("gpu_seqs_rate.py needs a HIP device: a rate is measured on the GPU or not at all")
    orc = rc.load_oracle()
    rng = np.random.default_rng(7)
    frames = rng.integers(400, 601, N_SEQS).astype(np.int32)
    seqs = [rng.standard_normal((n, FEATURES)).astype(np.float32) for n in frames]
    total = int(frames.sum())
    longest = int(frames.max())
    # (b)'s per-frame rows: recording k's frame t in row k, zeros once it has ended
    padded = np.zeros((longest, N_SEQS, FEATURES), np.float32)
    for k, s in enumerate(seqs):
        padded[:len(s), k] = s
    running = [np.flatnonzero(frames > t) for t in range(longest)]
    print("workload: %d recordings of %d .. %d frames of %d features (%d forward passes of one recording in all), %d classes"
          % (N_SEQS, frames.min(), frames.max(), FEATURES, total, CLASSES))
    print("(c) stages per segment: frames %d bytes a frame, answers %d, winners 1; default segment %d frames"
          % (4 * FEATURES, 4 * CLASSES, (2 << 20) // (256 * 4 * FEATURES)))
    goff, gsize = np.array([0], np.int32), np.array([CLASSES], np.int32)
    inp = (rc.c_float_p * N_SEQS)(*[rc.fptr(s) for s in seqs])
    for hidden in (512, 1024):
        net = amd.rnn_new(FEATURES, hidden, CLASSES, rc.FLAG_STANDARD, 11, None, 4, 1e-3, 0.9, 0.0, rc.RELU)
        amd.rnn_randomise_weights_auto(net)
        O = net.contents.o_size
        flags = net.contents.flags & ~(rc.FLAG_OWN_BPTT | rc.FLAG_OWN_WEIGHTS)
        err = np.zeros(CLASSES, np.float32)
        errp = rc.fptr(err)

        def loop(which):
            """(a): per frame rnn_opinion, the host's softmax_best_guess"""
            clones = [amd.rnn_clone(net, flags, rc.SUBSEED, None) for _ in which]
            last = amd.rnn_clone(net, flags, rc.SUBSEED, None)
            amd.rnn_opinion(last, rc.fptr(seqs[0][0]), 0.0)  # (the device image grows for the clones here)
            amd.rnn_amd_synchronize()
            prob = [np.zeros((frames[k], CLASSES), np.float32) for k in which]
            win = [np.zeros(frames[k], np.uint8) for k in which]
            t0 = time.perf_counter()
            for c, k, p, w in zip(clones, which, prob, win):
                real = rc.view(c.contents.real_inputs, FEATURES)
                s = seqs[k]
                for t in range(len(s)):
                    real[:] = s[t]
                    ans = amd.rnn_opinion(c, None, 0.0)
                    w[t] = orc.orc_softmax_best_guess(errp, ans, CLASSES)  # (leaves -softmax in err)
                    p[t] = -err
            amd.rnn_amd_synchronize()
            dt = time.perf_counter() - t0
            for c in [last] + clones[::-1]:
                amd.rnn_delete_net(c)
            return prob, win, dt

        def set_loop(upto):
            """(b): per frame one rnn_amd_set_opinion over 256 clones, the host's softmax_best_guess per running row"""
            cells = (rc.NetP * N_SEQS)()
            for k in range(N_SEQS):
                cells[k] = amd.rnn_clone(net, flags, rc.SUBSEED, None)
            handle = amd.rnn_amd_set_open(cells, N_SEQS)
            assert handle
            out = np.zeros((N_SEQS, O), np.float32)
            prob = [np.zeros((n, CLASSES), np.float32) for n in frames]
            win = [np.zeros(n, np.uint8) for n in frames]
            rows = [rc.fptr(out[k]) for k in range(N_SEQS)]
            amd.rnn_amd_synchronize()
            t0 = time.perf_counter()
            for t in range(upto):
                amd.rnn_amd_set_opinion(handle, rc.fptr(padded[t]), FEATURES, rc.fptr(out))
                for k in running[t]:
                    win[k][t] = orc.orc_softmax_best_guess(errp, rows[k], CLASSES)
                    prob[k][t] = -err
            amd.rnn_amd_synchronize()
            dt = time.perf_counter() - t0
            amd.rnn_amd_set_close(handle)
            for k in range(N_SEQS - 1, -1, -1):
                amd.rnn_delete_net(cells[k])
            return prob, win, dt

        def batched(segment):
            """(c): the arrays are the caller's and are made outside the clock, with guard entries behind them"""
            ans = [np.full(n * CLASSES + TRACE_GUARD, np.nan, np.float32) for n in frames]
            win = [np.full(n + TRACE_GUARD, 0xEE, np.uint8) for n in frames]
            ansp = (rc.c_float_p * N_SEQS)(*[rc.fptr(x) for x in ans])
            winp = (rc.c_u8_p * N_SEQS)(*[rc.u8ptr(x) for x in win])
            amd.rnn_amd_synchronize()
            t0 = time.perf_counter()
            r = amd.rnn_amd_run_sequences(scorer, inp, rc.iptr(frames), N_SEQS, FEATURES, 1, rc.iptr(goff), rc.iptr(gsize),
                                          None, None, segment, ansp, winp)
            amd.rnn_amd_synchronize()
            dt = time.perf_counter() - t0
            assert r == 0
            assert all(np.all(np.isnan(x[n * CLASSES:])) and np.all(y[n:] == 0xEE) for x, y, n in zip(ans, win, frames))
            return [x[:n * CLASSES].reshape(-1, CLASSES) for x, n in zip(ans, frames)], [y[:n] for y, n in zip(win, frames)], dt

        scorer = amd.rnn_clone(net, flags, rc.SUBSEED, None)  # hidden row zero, like the loops' fresh clones
        loop(list(range(4)))  # warm-up: every kernel of the three forms has run at its shapes
        set_loop(8)
        for segment in SEGMENTS:
            batched(segment)
        everything = list(range(N_SEQS))
        t_a, t_b, t_c = [], [], {s: [] for s in SEGMENTS}
        for r in range(ROUNDS):
            p_a, w_a, dt = loop(everything)
            t_a.append(dt)
            p_b, w_b, dt = set_loop(longest)
            t_b.append(dt)
            for segment in SEGMENTS:
                p_c, w_c, dt = batched(segment)
                t_c[segment].append(dt)
                if segment == SEGMENTS[0]:
                    p_0, w_0 = p_c, w_c
                else:
                    assert all(np.array_equal(x, y) for x, y in zip(p_c, p_0)) and all(np.array_equal(x, y) for x, y in zip(w_c, w_0))
        ra, rb = total / np.median(t_a), total / np.median(t_b)
        rcs = {s: total / np.median(t) for s, t in t_c.items()}
        print("hidden %4d: (a) loop of rnn_opinion + host softmax        %9.0f frames/s (%s s)" % (hidden, ra, " ".join("%.3f" % t for t in t_a)))
        print("hidden %4d: (b) loop of rnn_amd_set_opinion, 256 clones   %9.0f frames/s (%s s)" % (hidden, rb, " ".join("%.3f" % t for t in t_b)))
        for s in SEGMENTS:
            print("hidden %4d: (c) one rnn_amd_run_sequences, segment %-7s %9.0f frames/s (%s s)"
                  % (hidden, "default" if s == 0 else str(s), rcs[s], " ".join("%.4f" % t for t in t_c[s])))
        print("hidden %4d: (c default) / (a) = %.1f; (c default) / (b) = %.1f; %s"
              % (hidden, rcs[0] / ra, rcs[0] / rb, "; ".join("segment %d / default = %.3f" % (s, rcs[s] / rcs[0]) for s in SEGMENTS[1:])))
        flat_a, flat_b, flat_c = (np.concatenate(p) for p in (p_a, p_b, p_0))
        print("hidden %4d: (c) against (a): largest |difference| of a probability %.2e, %.4f of the winners the same; against (b): "
              "%.2e, %.4f; the three segment sizes give the same bits; class 1 wins %.3f of the frames"
              % (hidden, float(np.abs(flat_a - flat_c).max()), float(np.mean(np.concatenate(w_a) == np.concatenate(w_0))),
                 float(np.abs(flat_b - flat_c).max()), float(np.mean(np.concatenate(w_b) == np.concatenate(w_0))),
                 float(np.mean(np.concatenate(w_0) == 1))))
        amd.rnn_delete_net(scorer)
        amd.rnn_delete_net(net)


if __name__ == "__main__":
    main()
