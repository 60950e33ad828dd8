#!/usr/bin/env python3
"""Generates tests/golden/ref_live.npz and tests/golden/ref_header_offsets.txt: what the reference gives in the tests
that once called the compiled reference (oracle/_ref, built by oracle/Makefile) while they ran, recorded once so that
those tests need nothing outside the repository:

  * its struct sizes and, per activation and optimiser, its state at the start and after golden_cases.RUN_GENERATIONS
    generations of tests/test_oracle_vs_ref.py's run (the strict build);
  * the training entropy per window of tests/test_gpu_parity.py's hundred generations at hidden 1024 / 256 streams /
    depth 20 on erewhon.txt (the reference's -Ofast build, as that test drove it);
  * the mean error tools/pernet_rate.c prints linked against the reference, for golden_cases.PERNET_ARGS;
  * the offsetof / sizeof / enum table of golden_cases.header_offsets compiled against the reference's recur-nn.h.

Run where the reference's sources are, REF naming their directory as for oracle/Makefile:

    make -C oracle REF=<dir> && REF=<dir> python tests/golden/make_golden_live.py

The files are pure data (the reference's outputs); no reference source travels.
"""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import golden_cases as gc  # noqa: E402
import recur_ctypes as rc  # noqa: E402
import scenarios as sc  # noqa: E402


def run_cases(out):
    ref = rc.load_ref()
    out["sizeof_net"] = np.int64(ref.ref_sizeof_net())
    out["sizeof_bptt"] = np.int64(ref.ref_sizeof_bptt())
    text = sc.synthetic_text(gc.RUN_TEXT_LEN)
    for an, act in gc.RUN_ACTS.items():
        for mn, method in gc.RUN_METHODS.items():
            a = sc.ApiSet(ref, softmax_best_guess=ref.ref_softmax_best_guess, activation=act, **gc.RUN_KW)
            keys = sc.FLOAT_KEYS + sc.EXACT_KEYS
            for k, v in a.snapshot().items():  # (one start for all: the activation and the optimiser come later)
                if k in keys:
                    assert np.array_equal(out.setdefault("run.start." + k, v), v), k
            for i in range(gc.RUN_GENERATIONS):
                a.char_step(text, i, method, gc.RUN_MOMENTUM)
            for k, v in a.snapshot().items():
                if k in keys:
                    out["run.%s.%s.end.%s" % (an, mn, k)] = v
            a.close()


def hundred_generations(out):
    kw = gc.HUNDRED_KW
    text = rc.encode_erewhon(rc.load_amd())
    ref = rc.load_ref(fast=True)
    r = sc.ApiSet(ref, softmax_best_guess=ref.ref_softmax_best_guess, **kw)
    win, ent = gc.HUNDRED_WINDOW, []
    for w in range(gc.HUNDRED_GENERATIONS // win):
        lg = 0.0
        for i in range(w * win, (w + 1) * win):
            for e, _ in r.char_step(text, i, rc.WEIGHTED, gc.HUNDRED_MOMENTUM):
                l = 1.0 - e  # the probability given to the symbol that came (charmodel-helpers.h:11-13: capped log2)
                lg += -100.0 if l < 1e-30 else float(np.log2(np.float32(l)))
        ent.append(-lg / (win * kw["S"]))
        print("window %d: %.4f bits" % (w, ent[-1]), flush=True)
    r.close()
    out["hundred.entropy_per_window"] = np.array(ent, np.float64)


def pernet_rate(out, tmp):
    ref = os.path.join(rc.ROOT, "oracle", "_ref")
    exe = os.path.join(tmp, "pn_ref")
    subprocess.run(["gcc", "-O2", "-std=gnu11", "-D_GNU_SOURCE", "-I" + os.path.join(rc.ROOT, "include"),
                    os.path.join(rc.ROOT, "tools", "pernet_rate.c"), "-o", exe, "-L" + ref, "-lrecur_ref",
                    "-Wl,-rpath," + ref, "-lm"], check=True)
    got = []
    for args in gc.PERNET_ARGS:
        r = subprocess.run([exe] + list(args), capture_output=True, text=True, check=True, timeout=1800)
        got.append(float(re.search(r"mean error ([\d.]+)", r.stdout).group(1)))
    out["pernet.mean_error"] = np.array(got, np.float64)


def main():
    ref_dir = os.environ.get("REF")
    if not ref_dir or not os.path.exists(os.path.join(ref_dir, "recur-nn.h")) or not rc.have_ref():
        raise SystemExit("needs REF=<the reference's directory> and oracle/_ref built from it (make -C oracle REF=...)")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        with open(gc.HEADER_OFFSETS_GOLDEN, "w") as f:
            f.write(gc.header_offsets(tmp, ref_dir))
        run_cases(out)
        pernet_rate(out, tmp)
    hundred_generations(out)
    np.savez_compressed(gc.LIVE_GOLDEN, **out)
    print("wrote %s (%d arrays, %d bytes) and %s" % (gc.LIVE_GOLDEN, len(out), os.path.getsize(gc.LIVE_GOLDEN),
                                                    gc.HEADER_OFFSETS_GOLDEN))


if __name__ == "__main__":
    main()
