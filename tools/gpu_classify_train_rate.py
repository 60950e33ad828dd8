"""Rate probe: what a generation of gstclassify's trainer costs (maybe_learn, gstclassify.c:2180-2257) at BASELINE.json
configs[2]'s shape -- 32 features, 512 hidden, 2 classes in one group, BPTT depth 30, Nesterov with the soft start of 2000 --
with 128 channels (the configuration's), 8 and 1.  Routes, warmed up, alternated in the same process over the rounds and
timed by the host clock around REPEATS windows of WINDOW generations each (the same block again: its windows are labelled
alike) that end in one device synchronisation -- features and targets made before the clock starts:

  (a) the loop of rnn_amd_classify_generation with exact_gate 0: a momentum-only step where the reference makes none
  (b) the same loop with exact_gate 1: the reference's gate, two read-backs of the statistics per generation
  (c) one rnn_amd_classify_generations of WINDOW windows: the gate decided on the device
  (d) the same at blocks of 8 windows

A library without rnn_amd_classify_generations (RECUR_AMD_LIB pointing at a build of the commit before it) runs (a) and (b):
the baseline measured on code that is not the code under test.  Figures are generations per second (a generation is one
window of every channel and at most one update).  Not measured: balanced training (its draws are host work of a few
microseconds per channel either way), more than one class group, presynaptic noise (which takes the per-generation route),
real features (they are random; a tenth of the windows carry no label).

    python tools/gpu_classify_train_rate.py [rounds]          # writes what profiles/r16_classify_train_rate.txt holds
"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from recur_amd import api as rc  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
N_IN, HIDDEN, DEPTH, WINDOW, SMALL, REPEATS = 32, 512, 30, 64, 8, 10
CHANNELS = (128, 8, 1)
NEW_SET, NEW_CLASSIFY = ("rnn_amd_set_classify_steps",), ("rnn_amd_classify_generations",)
F = np.float32
SOFT = 2000.0


def load():
    """the library RECUR_AMD_LIB names, or the tree's; (lib, whether it has the call)"""
    lib = C.CDLL(os.environ.get("RECUR_AMD_LIB", rc.AMD_LIB))
    has = hasattr(lib, NEW_CLASSIFY[0])
    rc._bind(lib, rc.RNN_API)
    rc._bind(lib, rc.AMD_API, skip=() if has else NEW_SET)
    rc._bind(lib, rc.CLASSIFY_API, skip=() if has else NEW_CLASSIFY)
    return lib, has


def main():
    amd, has = load()
    if amd.rnn_amd_device_count() < 1:
        raise SystemExit("gpu_classify_train_rate.py needs a HIP device: a rate is measured on the GPU or not at all")
    # (which library, not where it lies: the line is kept in profiles/)
    print("library: %s (%s rnn_amd_classify_generations)"
          % ("the one RECUR_AMD_LIB names" if "RECUR_AMD_LIB" in os.environ else "the tree's", "with" if has else "WITHOUT"))
    print("workload: %d features, hidden %d, one group of 2 classes, depth %d, Nesterov, soft start %g; %d windows of %d generations "
          "per timing, %d rounds" % (N_IN, HIDDEN, DEPTH, SOFT, REPEATS, WINDOW, ROUNDS))
    goff, gsize = np.array([0], np.int32), np.array([2], np.int32)
    rs = np.random.default_rng(5)
    for channels in CHANNELS:
        x = np.ascontiguousarray((rs.standard_normal((WINDOW, channels, N_IN)) * 0.5).astype(F))
        tg = np.ascontiguousarray(rs.choice([0, 0, 0, 0, 1, 1, 1, 1, 1, -1], size=(WINDOW, channels, 1)).astype(np.int32))
        net = amd.rnn_new(N_IN, HIDDEN, 2, rc.FLAG_STANDARD, 11, None, DEPTH, 3e-4, 0.95, 0.0, rc.RELU)
        amd.rnn_randomise_weights_auto(net)
        nets = amd.rnn_new_training_set(net, channels)
        handle = amd.rnn_amd_set_open(nets, channels)
        assert handle

        def loop(n, exact):
            """(a), (b)"""
            amd.rnn_amd_synchronize()
            t0 = time.perf_counter()
            for t in range(n):
                k = t % WINDOW
                amd.rnn_amd_classify_generation(handle, rc.fptr(x[k]), N_IN, 1, rc.iptr(goff), rc.iptr(gsize), rc.iptr(tg[k]), None,
                                                None, rc.NESTEROV, SOFT, exact)
            amd.rnn_amd_synchronize()
            return time.perf_counter() - t0

        def blocks(n, block):
            """(c), (d)"""
            amd.rnn_amd_synchronize()
            t0 = time.perf_counter()
            for t in range(0, n, block):
                k, steps = t % WINDOW, min(block, n - t)
                amd.rnn_amd_classify_generations(handle, rc.fptr(x[k:]), N_IN, rc.iptr(tg[k:]), steps, 1, rc.iptr(goff),
                                                 rc.iptr(gsize), None, None, rc.NESTEROV, SOFT)
            amd.rnn_amd_synchronize()
            return time.perf_counter() - t0

        # warm-up: every kernel of every route has run at its shapes, the ring is full
        loop(DEPTH + 2, 0)
        loop(DEPTH + 2, 1)
        if has:
            blocks(DEPTH + 2, WINDOW)
            blocks(DEPTH + 2, SMALL)
        t_a, t_b, t_c, t_d = [], [], [], []
        for r in range(ROUNDS):
            t_a.append(loop(REPEATS * WINDOW, 0))
            t_b.append(loop(REPEATS * WINDOW, 1))
            if has:
                t_c.append(blocks(REPEATS * WINDOW, WINDOW))
                t_d.append(blocks(REPEATS * WINDOW, SMALL))

        def line(name, what, ts):
            print("%3d channels: (%s) %-62s %8.1f generations/s (%s s)"
                  % (channels, name, what, REPEATS * WINDOW / np.median(ts), " ".join("%.4f" % t for t in ts)))

        head = "%3d channels:" % channels
        line("a", "loop of rnn_amd_classify_generation, exact_gate 0", t_a)
        line("b", "loop of rnn_amd_classify_generation, exact_gate 1", t_b)
        if has:
            line("c", "one rnn_amd_classify_generations of %d windows" % WINDOW, t_c)
            line("d", "rnn_amd_classify_generations at blocks of %d" % SMALL, t_d)
            print("%s (c) / (a) = %.2f; (c) / (b) = %.2f; (d) / (b) = %.2f; (c) / (d) = %.3f"
                  % (head, np.median(t_a) / np.median(t_c), np.median(t_b) / np.median(t_c), np.median(t_b) / np.median(t_d),
                     np.median(t_d) / np.median(t_c)))
        amd.rnn_amd_set_close(handle)
        amd.rnn_delete_training_set(nets, channels, 0)
    sys.stdout.flush()


if __name__ == "__main__":
    main()
