"""Rate probe: continuing many prompts with one net, as the loop a caller writes without the batched call -- per prompt a
forward-only clone, rnn_amd_run_text(clone, prompt, plen, plen) to feed the prompt (rnn_char_prime's loop: five dependent
launches per symbol), then rnn_char_confabulate from the prompt's last symbol (every symbol a forward pass, a
synchronisation and the output row's way back, the draw on the host) -- against ONE rnn_amd_continue_texts call (the rows
side by side on the engine's scratch rows, longest first, prompt symbols fed and symbols drawn on the device by one launch
between two forward passes, one synchronisation per wave and one every 64 steps).  Workload: 256 prompts of 50 to 150
symbols from the erewhon text, each continued by 500 symbols, 42 symbols, no stop symbol, bias 0, at hidden 1024 and at
hidden 99.  Both forms are warmed up, timed by the host clock around work that ends in a device synchronisation, and
alternated in the same run; the figures are symbols per second (a symbol = one forward pass of one row, prompt symbols
and drawn ones alike).  The two forms' texts are valid samples of the same distributions but not the same bytes from the
first draw that falls within rounding of a boundary on (include/recur_amd.h): the probe prints how many of the 256 are
equal throughout, for the record, and judges nothing by it.

    python tools/gpu_continue_rate.py [rounds]          # writes what profiles/r07_continue_rate.txt holds

The process runs each hidden size in a child of its own under a time limit (a rate probe that hangs ends there, and
nothing more is started on the device after it)."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import recur_ctypes as rc  # noqa: E402
import scenarios as sc  # noqa: E402
from recur_amd.drivers import continue_texts  # noqa: E402

N_TEXTS, LENGTH, SYMBOLS = 256, 500, 42
PROMPT_LENS = [50 + (37 * k) % 101 for k in range(N_TEXTS)]  # 50 .. 150
STEP_LIMIT_S = {1024: 480, 99: 360}  # per hidden size: its training, warm-up and rounds


def init_rand64(seed):
    """recur-rng.h:33-43 in Python integers: the state a generator seeded `seed` starts from"""
    M = (1 << 64) - 1
    rot = lambda x, k: ((x << k) | (x >> (64 - k))) & M
    a, b, c, d = 0xF1EA5EED, seed, seed, seed
    for _ in range(20):
        e = (a - rot(b, 7)) & M
        a = b ^ rot(c, 13)
        b = (c + rot(d, 37)) & M
        c = (d + e) & M
        d = (e + a) & M
    return a, b, c, d


def measure(hidden, rounds):
    amd = rc.bind_char(rc.load_amd())
    if amd.rnn_amd_device_count() < 1:
        raise SystemExit("gpu_continue_rate.py needs a HIP device: a rate is measured on the GPU or not at all")
    text = rc.encode_erewhon(amd)
    alphabet = rc.default_text_alphabet(amd)
    a = sc.AmdBatchedSet(amd, input_size=SYMBOLS, hidden_size=hidden, output_size=SYMBOLS, S=4, D=10, learn_rate=1e-3, seed=1)
    a.load_text(np.ascontiguousarray(text[:20000]))
    for i in range(40):  # weights that are not the initial ones
        amd.rnn_amd_set_char_step(a.handle, i, rc.WEIGHTED, 0.9)
    flags = a.net.contents.flags & ~(rc.FLAG_OWN_BPTT | rc.FLAG_OWN_WEIGHTS)
    seeds = [1000 + k for k in range(N_TEXTS)]
    states = [init_rand64(s) for s in seeds]
    prompts = [np.ascontiguousarray(text[30000 + 211 * k:30000 + 211 * k + n]) for k, n in enumerate(PROMPT_LENS)]
    symbols = sum(PROMPT_LENS) - N_TEXTS + N_TEXTS * LENGTH  # forward passes: plen - 1 for the prompt, LENGTH for the draws

    def loop(which):
        """per prompt a fresh clone (hidden row zero, the row's generator), primed and sampled; the clones are made, seeded
        and deleted outside the clock"""
        clones = [amd.rnn_clone(a.net, flags, rc.SUBSEED, None) for _ in which]
        for c, k in zip(clones, which):
            r = c.contents.rng
            r.a, r.b, r.c, r.d = states[k]
            amd.rnn_amd_host_written(c, rc.RNN_AMD_STREAM)
        last = amd.rnn_clone(a.net, flags, rc.SUBSEED, None)
        amd.rnn_opinion(last, None, 0.0)  # (the device image grows for the clones here)
        amd.rnn_amd_synchronize()
        bufs = [C.create_string_buffer(LENGTH + 1) for _ in which]
        t0 = time.perf_counter()
        for c, b, k in zip(clones, bufs, which):
            p = prompts[k]
            amd.rnn_amd_run_text(c, rc.u8ptr(p), len(p), len(p))  # all but the last symbol fed, none scored
            amd.rnn_char_confabulate(c, b, LENGTH, LENGTH + 1, alphabet, 0.0, C.byref(C.c_int(int(p[-1]))), -1, -1)
        amd.rnn_amd_synchronize()
        dt = time.perf_counter() - t0
        for c in [last] + clones[::-1]:
            amd.rnn_delete_net(c)
        return [b.value for b in bufs], dt

    def batch():
        amd.rnn_amd_synchronize()
        t0 = time.perf_counter()
        texts, _ = continue_texts(amd, source, prompts, seeds, LENGTH)
        amd.rnn_amd_synchronize()
        return [bytes(rc.DEFAULT_CHARSET[s] for s in t) for t in texts], time.perf_counter() - t0

    source = amd.rnn_clone(a.net, flags, rc.SUBSEED, None)  # hidden row zero, like the loop's fresh clones
    loop(list(range(4)))  # warm-up: every kernel of both forms has run at its shapes
    batch()
    t_loop, t_batch = [], []
    for r in range(rounds):
        s_loop, dt = loop(list(range(N_TEXTS)))
        t_loop.append(dt)
        s_batch, dt = batch()
        t_batch.append(dt)
        print("hidden %4d, round %d: loop %.3f s, batch %.4f s" % (hidden, r, t_loop[-1], t_batch[-1]), flush=True)
    same = sum(x == y for x, y in zip(s_loop, s_batch))
    rl, rb = symbols / np.median(t_loop), symbols / np.median(t_batch)
    print("hidden %4d: loop of rnn_amd_run_text + rnn_char_confabulate %9.0f symbols/s (%s s), one rnn_amd_continue_texts "
          "%10.0f symbols/s (%s s): "
          "batch / loop = %.1f; %d of %d texts equal throughout" % (hidden, rl, " ".join("%.3f" % t for t in t_loop), rb,
                                                                    " ".join("%.4f" % t for t in t_batch), rb / rl, same, N_TEXTS))
    if rb <= rl:
        print("hidden %4d: the batch is NOT faster than the loop at this shape" % hidden)
    amd.rnn_delete_net(source)
    amd.rnn_char_free_alphabet(alphabet)
    a.close()


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--hidden":
        measure(int(sys.argv[2]), int(sys.argv[3]))
        return
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    print("workload: %d prompts of %d to %d symbols, each continued by %d symbols (%d forward passes of one row in all), "
          "%d symbols in the alphabet, bias 0, no stop symbol"
          % (N_TEXTS, min(PROMPT_LENS), max(PROMPT_LENS), LENGTH, sum(PROMPT_LENS) - N_TEXTS + N_TEXTS * LENGTH, SYMBOLS),
          flush=True)
    for hidden in (1024, 99):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--hidden", str(hidden), str(rounds)],
                               timeout=STEP_LIMIT_S[hidden])
        except subprocess.TimeoutExpired:
            raise SystemExit("hidden %d: not done within %d s; nothing more is started" % (hidden, STEP_LIMIT_S[hidden]))
        if r.returncode != 0:
            raise SystemExit("hidden %d: the step ended with status %d; nothing more is started" % (hidden, r.returncode))


if __name__ == "__main__":
    main()
