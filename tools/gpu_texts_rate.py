"""Rate probe: scoring many texts against one net, as a loop of rnn_amd_run_text on fresh forward-only clones (one text
after the other, five dependent launches per symbol) against ONE rnn_amd_run_texts call (the texts side by side on the
engine's scratch rows).  Workload: 42 symbols, 256 texts of 400 - 600 symbols from tests/golden/erewhon.txt, at hidden
1024 and at hidden 99.  Both forms are warmed up, timed by the host clock around work that ends in a device
synchronisation (every call of either form ends with one), and alternated in the same run; the figures are
symbols per second (a symbol = one forward pass of one text), the launches per symbol of both forms COUNTED from their
launch sequences (net_api.c run_text: assemble, GEMM, finalize, output layer, loss per symbol; texts_api.c run_wave: step
kernel, GEMM, finalize, output layer per step of the longest text, and one last step kernel), and the largest relative
difference between the two forms' sums.

    python tools/gpu_texts_rate.py [rounds]          # writes what profiles/r07_texts_rate.txt holds
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import recur_ctypes as rc  # noqa: E402
import scenarios as sc  # noqa: E402
from recur_amd.drivers import run_texts  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
N_TEXTS, SYMBOLS = 256, 42


def main():
    amd = rc.bind_char(rc.load_amd())
    if amd.rnn_amd_device_count() < 1:
        raise SystemExit("gpu_texts_rate.py needs a HIP device: a rate is measured on the GPU or not at all")
    text = rc.encode_erewhon(amd)
    rng = np.random.default_rng(7)
    lens = rng.integers(400, 601, N_TEXTS)
    starts = rng.integers(30000, len(text) - 601, N_TEXTS)
    texts = [np.ascontiguousarray(text[a:a + n]) for a, n in zip(starts, lens)]
    symbols = int((lens - 1).sum())
    steps = int(lens.max()) - 1
    print("workload: %d texts of %d .. %d symbols (%d forward passes of one text in all), %d symbols in the alphabet"
          % (N_TEXTS, lens.min(), lens.max(), symbols, SYMBOLS))
    print("launches per symbol, counted: loop %.2f (5 per symbol), batch %.4f (4 per step of the longest text + 1 = %d launches)"
          % (5.0, (4 * steps + 1) / symbols, 4 * steps + 1))
    for hidden in (1024, 99):
        a = sc.AmdBatchedSet(amd, input_size=SYMBOLS, hidden_size=hidden, output_size=SYMBOLS, S=4, D=10, learn_rate=1e-3, seed=1)
        a.load_text(np.ascontiguousarray(text[:20000]))
        for i in range(40):  # weights that are not the initial ones
            amd.rnn_amd_set_char_step(a.handle, i, rc.WEIGHTED, 0.9)
        flags = a.net.contents.flags & ~(rc.FLAG_OWN_BPTT | rc.FLAG_OWN_WEIGHTS)

        def loop(which):
            """the loop of rnn_amd_run_text, a fresh clone per text; the clones are made and deleted outside the clock"""
            clones = [amd.rnn_clone(a.net, flags, rc.SUBSEED, None) for _ in which]
            last = amd.rnn_clone(a.net, flags, rc.SUBSEED, None)
            amd.rnn_amd_run_text(last, rc.u8ptr(texts[0]), 2, 0)  # (the device image grows for the clones here)
            amd.rnn_amd_synchronize()
            t0 = time.perf_counter()
            sums = [amd.rnn_amd_run_text(c, rc.u8ptr(texts[k]), len(texts[k]), 0) for c, k in zip(clones, which)]
            amd.rnn_amd_synchronize()
            dt = time.perf_counter() - t0
            for c in [last] + clones[::-1]:
                amd.rnn_delete_net(c)
            return np.array(sums), dt

        def batch():
            amd.rnn_amd_synchronize()
            t0 = time.perf_counter()
            sums = run_texts(amd, scorer, texts)
            amd.rnn_amd_synchronize()
            return sums, time.perf_counter() - t0

        scorer = amd.rnn_clone(a.net, flags, rc.SUBSEED, None)  # hidden row zero, like the loop's fresh clones
        loop(list(range(8)))  # warm-up: every kernel of both forms has run at its shapes
        batch()
        everything = list(range(N_TEXTS))
        t_loop, t_batch = [], []
        for r in range(ROUNDS):
            s_loop, dt = loop(everything)
            t_loop.append(dt)
            s_batch, dt = batch()
            t_batch.append(dt)
        rel = float(np.max(np.abs(s_loop - s_batch) / np.abs(s_loop)))
        rl, rb = symbols / np.median(t_loop), symbols / np.median(t_batch)
        print("hidden %4d: loop of rnn_amd_run_text %9.0f symbols/s (%s s), one rnn_amd_run_texts %10.0f symbols/s (%s s): "
              "batch / loop = %.1f; largest relative difference of the sums %.2e (mean entropy %.3f bits)"
              % (hidden, rl, " ".join("%.3f" % t for t in t_loop), rb, " ".join("%.4f" % t for t in t_batch), rb / rl, rel,
                 float(-s_batch.sum() / symbols)))
        if rb <= rl:
            print("hidden %4d: the batch is NOT faster than the loop at this shape" % hidden)
        amd.rnn_delete_net(scorer)
        a.close()


if __name__ == "__main__":
    main()
