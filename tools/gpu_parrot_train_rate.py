"""Rate probe: what a generation of parrot's trainer costs (maybe_learn, gstparrot.c:487-554), 256 channels of 256 MDCT bins
(a net of 256 inputs and 256 outputs) at BPTT depth 30, hidden 199 (the plugin's), 512 and 1024.  Four routes, warmed up,
(a) to (c) alternated in the same process over the rounds and timed by the host clock around WINDOW generations that end in
a device synchronisation -- the caller's arrays made before the clock starts:

  (a) today's loop, what a caller had to do before the library knew the loss: per generation rnn_bptt_clear_deltas,
      rnn_amd_set_advance, rnn_amd_set_opinion that brings 256 x 256 answers back -- which synchronises --, fast_tanhf and
      (1 - a a)(target - a) in numpy float32 on the host, rnn_amd_set_put_o_error, rnn_amd_set_calc_deltas,
      rnn_apply_learning
  (b) one rnn_amd_set_dense_step_tanh per generation (host rows up per generation, nothing back)
  (c) one rnn_amd_set_dense_steps_tanh of WINDOW generations (the block up once)
  (d) (b) with RECUR_AMD_DENSE_TOP=0: the loss and the top backprop as launches of their own.  The switch is read once per
      process, so (d) runs in a child process of its own behind the others, the same rounds and windows.

A library without rnn_amd_set_dense_step_tanh (RECUR_AMD_LIB pointing at a build of the commit before it) runs (a) alone:
the baseline measured on code that is not the code under test.  Figures are generations per second (a generation is 256
channel-steps).  Not measured: other channel counts, blocks longer than WINDOW, the conditioning.

    python tools/gpu_parrot_train_rate.py [rounds]          # writes what profiles/r14_parrot_train_rate.txt holds
"""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from recur_amd import api as rc  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
CHILD = len(sys.argv) > 2 and sys.argv[2] == "step-only"
CHANNELS, FEATS, DEPTH, WINDOW = 256, 256, 30, 64
HIDDEN = (199, 512, 1024)
NEW = ("rnn_amd_set_tanh_error", "rnn_amd_set_opinion_tanh_error", "rnn_amd_set_dense_step_tanh", "rnn_amd_set_dense_steps_tanh")
F = np.float32
MOMENTUM = 0.95


def load():
    """the library RECUR_AMD_LIB names, or the tree's; (lib, whether it has the calls)"""
    lib = C.CDLL(os.environ.get("RECUR_AMD_LIB", rc.AMD_LIB))
    has = hasattr(lib, "rnn_amd_set_dense_step_tanh")
    rc._bind(lib, rc.RNN_API)
    rc._bind(lib, rc.AMD_API, skip=() if has else NEW)
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
        raise SystemExit("gpu_parrot_train_rate.py needs a HIP device: a rate is measured on the GPU or not at all")
    top = os.environ.get("RECUR_AMD_DENSE_TOP", "1")
    if not CHILD:
        # (which library, not where it lies: the line is kept in profiles/)
        print("library: %s (%s rnn_amd_set_dense_step_tanh)"
              % ("the one RECUR_AMD_LIB names" if "RECUR_AMD_LIB" in os.environ else "the tree's", "with" if has else "WITHOUT"))
        print("workload: %d channels of %d bins, depth %d, windows of %d generations, %d rounds; a frame is %d bytes"
              % (CHANNELS, FEATS, DEPTH, WINDOW, ROUNDS, 4 * CHANNELS * FEATS))
    frames = np.ascontiguousarray(np.random.default_rng(5).uniform(-0.5, 0.5, (WINDOW + 1, CHANNELS, FEATS)).astype(F))
    for hidden in HIDDEN:
        net = amd.rnn_new(FEATS, hidden, FEATS, rc.FLAG_STANDARD | rc.FLAG_ADAPTIVE_MIN_ERROR, 11, None, DEPTH, 1e-6, MOMENTUM,
                          0.0, rc.RELU)
        amd.rnn_randomise_weights_auto(net)
        nets = amd.rnn_new_training_set(net, CHANNELS)
        handle = amd.rnn_amd_set_open(nets, CHANNELS)
        assert handle
        O = net.contents.o_size
        out = np.zeros((CHANNELS, O), F)
        err = np.zeros((CHANNELS, O), F)

        def loop_host(n):
            """(a): -> (the loop's time, the host's time in it)"""
            amd.rnn_amd_synchronize()
            host = 0.0
            t0 = time.perf_counter()
            for t in range(n):
                amd.rnn_bptt_clear_deltas(net)
                amd.rnn_amd_set_advance(handle)
                amd.rnn_amd_set_opinion(handle, rc.fptr(frames[t]), FEATS, rc.fptr(out))
                h0 = time.perf_counter()
                a = np_tanh(out[:, :FEATS])
                err[:, :FEATS] = (F(1.0) - a * a) * (frames[t + 1] - a)
                host += time.perf_counter() - h0
                amd.rnn_amd_set_put_o_error(handle, rc.fptr(err), O)
                amd.rnn_amd_set_calc_deltas(handle, 1, None, None)
                amd.rnn_apply_learning(net, rc.WEIGHTED, MOMENTUM)
            amd.rnn_amd_synchronize()
            return time.perf_counter() - t0, host

        def loop_step(n):
            """(b), (d)"""
            amd.rnn_amd_synchronize()
            t0 = time.perf_counter()
            for t in range(n):
                amd.rnn_amd_set_dense_step_tanh(handle, rc.fptr(frames[t]), FEATS, rc.fptr(frames[t + 1]), FEATS, FEATS, rc.WEIGHTED,
                                                MOMENTUM)
            amd.rnn_amd_synchronize()
            return time.perf_counter() - t0

        def one_call(n):
            """(c)"""
            amd.rnn_amd_synchronize()
            t0 = time.perf_counter()
            amd.rnn_amd_set_dense_steps_tanh(handle, rc.fptr(frames), FEATS, n, FEATS, rc.WEIGHTED, MOMENTUM, 0)
            amd.rnn_amd_synchronize()
            return time.perf_counter() - t0

        # warm-up: every kernel of every route has run at its shapes, the ring is full
        if not CHILD:
            loop_host(DEPTH + 2)
        if has:
            loop_step(DEPTH + 2)
            if not CHILD:
                one_call(DEPTH + 2)
        t_a, h_a, t_b, t_c = [], [], [], []
        for r in range(ROUNDS):
            if not CHILD:
                dt, host = loop_host(WINDOW)
                t_a.append(dt)
                h_a.append(host)
            if has:
                t_b.append(loop_step(WINDOW))
                if not CHILD:
                    t_c.append(one_call(WINDOW))

        def line(name, what, ts):
            print("hidden %4d: (%s) %-62s %8.1f generations/s (%s s)"
                  % (hidden, name, what, WINDOW / np.median(ts), " ".join("%.4f" % t for t in ts)))

        if CHILD:
            line("d", "(b) with RECUR_AMD_DENSE_TOP=%s, a process of its own" % top, t_b)
        else:
            line("a", "today's loop: opinion fetched, numpy loss, put_o_error", t_a)
            print("hidden %4d:     the host's share of (a) %.1f %% (%s s)"
                  % (hidden, 100.0 * np.median(h_a) / np.median(t_a), " ".join("%.4f" % t for t in h_a)))
            if has:
                line("b", "rnn_amd_set_dense_step_tanh per generation", t_b)
                line("c", "one rnn_amd_set_dense_steps_tanh of %d generations" % WINDOW, t_c)
                print("hidden %4d: (b) / (a) = %.2f; (c) / (a) = %.2f; (c) / (b) = %.3f"
                      % (hidden, np.median(t_a) / np.median(t_b), np.median(t_a) / np.median(t_c), np.median(t_b) / np.median(t_c)))
        if not CHILD:
            st = rc.AmdStats()
            amd.rnn_amd_set_read_stats(handle, C.byref(st), 1)
            gens = (DEPTH + 2) * (3 if has else 1) + ROUNDS * WINDOW * (3 if has else 1)
            print("hidden %4d:     executed BPTT steps per channel-step, all routes: %.1f of %d"
                  % (hidden, st.bptt_depth_sum / (gens * CHANNELS), DEPTH))
        amd.rnn_amd_set_close(handle)
        amd.rnn_delete_training_set(nets, CHANNELS, 0)
    sys.stdout.flush()
    if has and not CHILD:
        env = dict(os.environ, RECUR_AMD_DENSE_TOP="0")
        subprocess.run([sys.executable, os.path.abspath(__file__), str(ROUNDS), "step-only"], env=env, check=True, timeout=600)


if __name__ == "__main__":
    main()
