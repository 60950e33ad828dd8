"""Rate probe: what a generation of rnnca's trainer costs (maybe_learn, gstrnnca.c:718-750) on the default 35-input pattern
on 144 x 96, BPTT depth 10, with 200 trainers (the plugin's) and 512 (BASELINE's rnnca generation), hidden 512 and 2048.
Three routes, warmed up, alternated in the same process over the rounds and timed by the host clock around WINDOW
generations that end in a device synchronisation -- the film and the positions made before the clock starts:

  (a) today's loop: per generation every trainer's input row gathered from the frame before and its three target bytes read
      from the frame now, in numpy on the host (fill_net_inputs, gstrnnca.c:669-691; vectorised over the trainers), then
      rnn_amd_set_dense_step_sigmoid_mse.  The host's share -- the gather -- is printed separately.
  (b) one rnn_amd_set_automaton_steps of WINDOW generations: the film up once, the rows gathered on the device
  (c) the same at blocks of 8 generations

A library without rnn_amd_set_automaton_steps (RECUR_AMD_LIB pointing at a build of the commit before it) runs (a) alone:
the baseline measured on code that is not the code under test.  Figures are generations per second (a generation is one
update from all trainers).  Not measured: other grids and patterns, moving trainers (the positions are fixed per window,
handed over per generation all the same), the conditioning, presynaptic noise, a real film (the bytes are random).

    python tools/gpu_automaton_train_rate.py [rounds]          # writes what profiles/r15_automaton_train_rate.txt holds
"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from recur_amd import api as rc  # noqa: E402
from recur_amd.drivers import AutomatonGeometry, parse_offsets  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
WIDTH, HEIGHT, DEPTH, WINDOW, SMALL = 144, 96, 10, 64, 8
SIZES = ((200, 512), (512, 512), (200, 2048), (512, 2048))      # (trainers, hidden)
NEW = ("rnn_amd_set_automaton_steps",)
F = np.float32
MOMENTUM = 0.5


def load():
    """the library RECUR_AMD_LIB names, or the tree's; (lib, whether it has the call)"""
    lib = C.CDLL(os.environ.get("RECUR_AMD_LIB", rc.AMD_LIB))
    has = hasattr(lib, NEW[0])
    rc._bind(lib, rc.RNN_API)
    rc._bind(lib, rc.AMD_API, skip=() if has else NEW)
    return lib, has


def host_rows(frame, after, xy, ys, cs):
    """fill_net_inputs and the targets for all trainers at once, clamped edges, two position inputs: numpy float32"""
    recip = F(1.0) / F(255.0)
    x, y = xy[:, 0], xy[:, 1]
    planes, nxt = frame.reshape(3, -1), after.reshape(3, -1)

    def at(dx, dy):
        return np.clip(y + dy, 0, HEIGHT - 1) * WIDTH + np.clip(x + dx, 0, WIDTH - 1)

    cols = [planes[0, at(dx, dy)].astype(F) * recip for dx, dy in ys]
    for dx, dy in cs:
        a = at(dx, dy)
        cols += [planes[1, a].astype(F) * recip, planes[2, a].astype(F) * recip]
    cols += [x.astype(F) * F(1.0) / F(WIDTH), y.astype(F) * F(1.0) / F(HEIGHT)]
    own = y * WIDTH + x
    return np.ascontiguousarray(np.stack(cols, axis=1), F), np.ascontiguousarray(nxt[:, own].T.astype(F) * recip, F)


def main():
    amd, has = load()
    if amd.rnn_amd_device_count() < 1:
        raise SystemExit("gpu_automaton_train_rate.py needs a HIP device: a rate is measured on the GPU or not at all")
    # (which library, not where it lies: the line is kept in profiles/)
    print("library: %s (%s rnn_amd_set_automaton_steps)"
          % ("the one RECUR_AMD_LIB names" if "RECUR_AMD_LIB" in os.environ else "the tree's", "with" if has else "WITHOUT"))
    print("workload: %d x %d, the default pattern (35 inputs), depth %d, windows of %d generations, %d rounds; a frame is %d bytes"
          % (WIDTH, HEIGHT, DEPTH, WINDOW, ROUNDS, 3 * WIDTH * HEIGHT))
    ys, cs = parse_offsets(amd, "Y00120111C0111")
    geometry = AutomatonGeometry(WIDTH, HEIGHT, ys, cs, 2, 1)
    rs = np.random.default_rng(5)
    film = np.ascontiguousarray(rs.integers(0, 256, (WINDOW + 1, 3, HEIGHT, WIDTH), dtype=np.uint8))
    for trainers, hidden in SIZES:
        xy = np.ascontiguousarray(np.stack([rs.integers(2, WIDTH - 2, trainers), rs.integers(2, HEIGHT - 2, trainers)], axis=1),
                                  np.int32)
        xys = np.ascontiguousarray(np.broadcast_to(xy, (WINDOW, trainers, 2)))
        net = amd.rnn_new(geometry.input_size, hidden, 3, rc.FLAG_STANDARD, 11, None, DEPTH, 1e-6, MOMENTUM, 0.0, rc.RELU)
        amd.rnn_randomise_weights_auto(net)
        nets = amd.rnn_new_training_set(net, trainers)
        handle = amd.rnn_amd_set_open(nets, trainers)
        assert handle

        def loop_host(n):
            """(a): -> (the loop's time, the host's time in it)"""
            amd.rnn_amd_synchronize()
            host = 0.0
            t0 = time.perf_counter()
            for t in range(n):
                h0 = time.perf_counter()
                x, tg = host_rows(film[t], film[t + 1], xys[t], ys, cs)
                host += time.perf_counter() - h0
                amd.rnn_amd_set_dense_step_sigmoid_mse(handle, rc.fptr(x), x.shape[1], rc.fptr(tg), 3, 3, rc.WEIGHTED, MOMENTUM)
            amd.rnn_amd_synchronize()
            return time.perf_counter() - t0, host

        def blocks(n, block):
            """(b), (c)"""
            amd.rnn_amd_synchronize()
            t0 = time.perf_counter()
            for t in range(0, n, block):
                steps = min(block, n - t)
                amd.rnn_amd_set_automaton_steps(handle, C.byref(geometry.struct), rc.u8ptr(film[t:]), rc.iptr(xys[t:]), 1, steps,
                                                0, rc.WEIGHTED, MOMENTUM, 0.0, 0)
            amd.rnn_amd_synchronize()
            return time.perf_counter() - t0

        # warm-up: every kernel of every route has run at its shapes, the ring is full
        loop_host(DEPTH + 2)
        if has:
            blocks(DEPTH + 2, WINDOW)
            blocks(DEPTH + 2, SMALL)
        t_a, h_a, t_b, t_c = [], [], [], []
        for r in range(ROUNDS):
            dt, host = loop_host(WINDOW)
            t_a.append(dt)
            h_a.append(host)
            if has:
                t_b.append(blocks(WINDOW, WINDOW))
                t_c.append(blocks(WINDOW, SMALL))

        def line(name, what, ts):
            print("%3d trainers, hidden %4d: (%s) %-58s %8.1f generations/s (%s s)"
                  % (trainers, hidden, name, what, WINDOW / np.median(ts), " ".join("%.4f" % t for t in ts)))

        head = "%3d trainers, hidden %4d:" % (trainers, hidden)
        line("a", "today's loop: numpy gather, rnn_amd_set_dense_step_sigmoid_mse", t_a)
        print("%s     the host's share of (a) %.1f %% (%s s)"
              % (head, 100.0 * np.median(h_a) / np.median(t_a), " ".join("%.4f" % t for t in h_a)))
        if has:
            line("b", "one rnn_amd_set_automaton_steps of %d generations" % WINDOW, t_b)
            line("c", "rnn_amd_set_automaton_steps at blocks of %d" % SMALL, t_c)
            print("%s (b) / (a) = %.2f; (c) / (a) = %.2f; (b) / (c) = %.3f"
                  % (head, np.median(t_a) / np.median(t_b), np.median(t_a) / np.median(t_c), np.median(t_c) / np.median(t_b)))
        amd.rnn_amd_set_close(handle)
        amd.rnn_delete_training_set(nets, trainers, 0)
    sys.stdout.flush()


if __name__ == "__main__":
    main()
