"""Rate probe: what it costs to dream parrot's player, 256 channels of 256 MDCT bins (a net of 256 inputs and 256 outputs)
for 256 frames from a zero row, each channel fed its own last answer (fill_audio_chunk, gstparrot.c:556-583).  Five routes,
warmed up, alternated in the same process and timed by the host clock around work that ends in a device synchronisation --
the caller's arrays made before the clock starts:

  (a) today's loop: per frame one rnn_amd_set_opinion over 256 forward-only clones uploads the rows, runs the pass and
      brings 256 x 256 answers back -- which synchronises --, and the host applies the tanh rule and the noise product in
      numpy float32.  The host's noise is numpy's standard_normal: a stand-in with the cost of a fast host generator (the
      reference's, restated in Python, would cost more than everything else together), so the host's share reported here
      is a lower bound and the frames are another film than (c)'s.
  (b) the per-net loop: per frame 256 calls of rnn_opinion, one per clone, the same host work.  It is timed over B_FRAMES
      frames, not 256: its rate does not depend on the count.
  (c) one rnn_amd_dream_sequences with noise 1 at the default segment (64 frames of this size: four segments)
  (d) the same with noise 0: nothing is drawn; (c) - (d) per frame is what the draws cost
  (e) (c) at segments of 1 frame: a copy and a synchronisation per frame

A library without rnn_amd_dream_sequences (RECUR_AMD_LIB pointing at a build of the commit before it) runs (a) and (b)
alone: the baseline measured on code that is not the code under test.
The loops are driven from Python through ctypes, as every probe here is; clones and the set are made outside the clock.
At hidden 512, then 1024, seeded weights.  Figures are frames per second.

    python tools/gpu_dream_rate.py [rounds]          # writes what profiles/r13_dream_rate.txt holds
"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from recur_amd import api as rc  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
CHANNELS, FEATS, FRAMES, B_FRAMES = 256, 256, 256, 32
F = np.float32
GUARD = 4


def load():
    """the library RECUR_AMD_LIB names, or the tree's; (lib, whether it has the one call)"""
    lib = C.CDLL(os.environ.get("RECUR_AMD_LIB", rc.AMD_LIB))
    has = hasattr(lib, "rnn_amd_dream_sequences")
    rc._bind(lib, rc.RNN_API)
    rc._bind(lib, rc.AMD_API, skip=() if has else ("rnn_amd_dream_sequences",))
    return lib, has


def np_tanh(x):
    """dream_rule.h's dream_tanh in numpy float32 (badmaths.h:55-68)"""
    x2 = x * x
    a = x * (F(135135.0) + x2 * (F(17325.0) + x2 * (F(378.0) + x2)))
    b = F(135135.0) + x2 * (F(62370.0) + x2 * (F(3150.0) + x2 * F(28.0)))
    return np.where(x <= F(-4.97), F(-1.0), np.where(x >= F(4.97), F(1.0), a / b)).astype(F)


def main():
    amd, has = load()
    if amd.rnn_amd_device_count() < 1:
        raise SystemExit("gpu_dream_rate.py needs a HIP device: a rate is measured on the GPU or not at all")
    print("library: %s (%s rnn_amd_dream_sequences)" % (os.environ.get("RECUR_AMD_LIB", "the tree's"), "with" if has else "WITHOUT"))
    print("workload: %d channels of %d bins, %d frames from a zero row; a frame is %d bytes each way in (a)"
          % (CHANNELS, FEATS, FRAMES, 4 * CHANNELS * FEATS))
    u64p, ctxp = C.POINTER(C.c_uint64), C.POINTER(rc.RandCtx)
    for hidden in (512, 1024):
        net = amd.rnn_new(FEATS, hidden, FEATS, rc.FLAG_STANDARD, 11, None, 4, 1e-3, 0.9, 0.0, rc.RELU)
        amd.rnn_randomise_weights_auto(net)
        O = net.contents.o_size
        flags = net.contents.flags & ~(rc.FLAG_OWN_BPTT | rc.FLAG_OWN_WEIGHTS)
        clones = (rc.NetP * CHANNELS)()
        for k in range(CHANNELS):
            clones[k] = amd.rnn_clone(net, flags, rc.SUBSEED, None)
        handle = amd.rnn_amd_set_open(clones, CHANNELS)
        assert handle
        out = np.zeros((CHANNELS, O), F)
        first = np.zeros((CHANNELS, FEATS), F)
        seeds = np.arange(CHANNELS, dtype=np.uint64) + np.uint64(1)
        host_rng = np.random.default_rng(3)

        def host_rule(raw, frames, t):
            a = np_tanh(raw)
            frames[t] = a
            return (a * (F(1.0) + host_rng.standard_normal(a.shape, dtype=F))).astype(F)

        def loop_set(n_frames):
            """(a): returns (the frames, the loop's time, the host's time in it)"""
            frames = np.zeros((n_frames, CHANNELS, FEATS), F)
            x = first.copy()
            amd.rnn_amd_synchronize()
            host = 0.0
            t0 = time.perf_counter()
            for t in range(n_frames):
                amd.rnn_amd_set_opinion(handle, rc.fptr(x), FEATS, rc.fptr(out))
                h0 = time.perf_counter()
                x = host_rule(out[:, :FEATS], frames, t)
                host += time.perf_counter() - h0
            amd.rnn_amd_synchronize()
            return frames, time.perf_counter() - t0, host

        def loop_nets(n_frames):
            """(b)"""
            frames = np.zeros((n_frames, CHANNELS, FEATS), F)
            x = first.copy()
            raw = np.zeros((CHANNELS, FEATS), F)
            amd.rnn_amd_synchronize()
            host = 0.0
            t0 = time.perf_counter()
            for t in range(n_frames):
                for k in range(CHANNELS):
                    raw[k] = rc.view(amd.rnn_opinion(clones[k], rc.fptr(x[k]), 0.0), O)[:FEATS]
                h0 = time.perf_counter()
                x = host_rule(raw, frames, t)
                host += time.perf_counter() - h0
            amd.rnn_amd_synchronize()
            return frames, time.perf_counter() - t0, host

        def one_call(noise, segment):
            """(c), (d), (e): the arrays are the caller's and are made outside the clock, with guard floats behind them"""
            frames = np.full(FRAMES * CHANNELS * FEATS + GUARD, np.nan, F)
            amd.rnn_amd_synchronize()
            t0 = time.perf_counter()
            r = amd.rnn_amd_dream_sequences(net, rc.fptr(first), FEATS, CHANNELS, FRAMES, noise, seeds.ctypes.data_as(u64p), None,
                                            None, None, segment, rc.fptr(frames), None, None)
            amd.rnn_amd_synchronize()
            dt = time.perf_counter() - t0
            assert r == 0 and np.all(np.isnan(frames[FRAMES * CHANNELS * FEATS:]))
            return frames[:FRAMES * CHANNELS * FEATS].reshape(FRAMES, CHANNELS, FEATS), dt

        calls = [("c", 1.0, 0), ("d", 0.0, 0), ("e", 1.0, 1)] if has else []
        # warm-up: every kernel of every route has run at its shapes
        f_a, _, _ = loop_set(2)
        f_n, _, _ = loop_nets(1)
        kept = {name: one_call(noise, segment)[0] for name, noise, segment in calls}
        t_a, h_a, t_n, h_n, t_c = [], [], [], [], {name: [] for name, _, _ in calls}
        for r in range(ROUNDS):
            _, dt, host = loop_set(FRAMES)
            t_a.append(dt)
            h_a.append(host)
            _, dt, host = loop_nets(B_FRAMES)
            t_n.append(dt)
            h_n.append(host)
            for name, noise, segment in calls:
                f, dt = one_call(noise, segment)
                t_c[name].append(dt)
                assert np.array_equal(f, kept[name])   # the same bits every round
        ra, rn = FRAMES / np.median(t_a), B_FRAMES / np.median(t_n)
        print("hidden %4d: (a) today's loop, set_opinion + numpy tanh and noise %8.1f frames/s (%s s); the host's share %.1f %% (%s s)"
              % (hidden, ra, " ".join("%.3f" % t for t in t_a), 100.0 * np.median(h_a) / np.median(t_a),
                 " ".join("%.3f" % t for t in h_a)))
        print("hidden %4d: (b) the per-net loop, %d x rnn_opinion per frame, %d frames %8.1f frames/s (%s s); the host's share %.1f %%"
              % (hidden, CHANNELS, B_FRAMES, rn, " ".join("%.3f" % t for t in t_n), 100.0 * np.median(h_n) / np.median(t_n)))
        print("hidden %4d: (a) / (b) = %.2f" % (hidden, ra / rn))
        if has:
            rate = {name: FRAMES / np.median(t) for name, t in t_c.items()}
            what = {"c": "noise 1, default segment", "d": "noise 0, default segment", "e": "noise 1, segments of 1 frame"}
            for name, _, _ in calls:
                print("hidden %4d: (%s) one rnn_amd_dream_sequences, %-28s %8.1f frames/s (%s s)"
                      % (hidden, name, what[name], rate[name], " ".join("%.4f" % t for t in t_c[name])))
            per = {name: 1e6 * np.median(t) / FRAMES for name, t in t_c.items()}
            print("hidden %4d: (c) / (a) = %.2f; (c) / (b) = %.1f; (d) / (c) = %.3f; (e) / (c) = %.3f; per frame (c) %.1f us, "
                  "(d) %.1f us: the draws cost %.1f us a frame"
                  % (hidden, rate["c"] / ra, rate["c"] / rn, rate["d"] / rate["c"], rate["e"] / rate["c"], per["c"], per["d"],
                     per["c"] - per["d"]))
            print("hidden %4d: frame 0 of (c), (d) and (e) the same bits: %s; (e) is (c) bit for bit: %s; frame 0 of (c) against "
                  "frame 0 of (a): largest difference %.3g; (c)'s last frame: largest |value| %.3g, %d distinct values"
                  % (hidden, np.array_equal(kept["c"][0], kept["d"][0]) and np.array_equal(kept["c"][0], kept["e"][0]),
                     np.array_equal(kept["c"], kept["e"]), float(np.abs(kept["c"][0] - f_a[0]).max()),
                     float(np.abs(kept["c"][-1]).max()), len(np.unique(kept["c"][-1]))))
        amd.rnn_amd_set_close(handle)
        for k in range(CHANNELS - 1, -1, -1):
            amd.rnn_delete_net(clones[k])
        amd.rnn_delete_net(net)


if __name__ == "__main__":
    main()
