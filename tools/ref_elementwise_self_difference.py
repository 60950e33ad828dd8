"""CPU probe (build container, where oracle/_ref exists): what does "1e-4 relative" mean ELEMENT BY ELEMENT for this
algorithm?  The reference against ITSELF -- its strict-IEEE build (oracle/_ref/librecur_ref.so) against its own -Ofast
build (librecur_ref_fast.so: reassociated sums, fused multiply-adds) -- ONE generation deep from bit-identical state, at
several shapes; per array: the 2-norm error, the largest-element error (both relative to the array), and the worst
element-wise relative error over the elements that are not small, |b| >= floor * max|b|, for floor = 1e-1, 1e-2, 1e-3.
Context: VERDICT.md round 4, weak spot 2 ("an element 100x smaller than the array's largest may be 1 % off and pass").
A sum of K products carries ~sqrt(K) eps of ITS LARGEST partial sums as rounding, not of its own value: an element that
cancelled down to 1e-3 of the array's largest differs by 1e-4 .. 1e-3 of itself between any two summation orders --
including the reference's two builds.  The numbers printed here are what tests/replay.py's element-wise bar is set by.
usage: python tools/ref_elementwise_self_difference.py [H,S,D,lr,warm[,activation[,variance[,seed]]] ...]
(without arguments: the shapes the bar was set by; with them: those shapes instead, e.g. 130,40,6,1e-5,9,5,0.1,3 for a
RECLIP20 net with large initial weights, whose units reach the ceiling)"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np
import recur_ctypes as rc, scenarios as sc

strict, fast = rc.load_ref(), rc.load_ref(fast=True)
text = sc.synthetic_text(6000)
KEYS = ["ih_delta", "ho_delta", "ih_w", "ho_w", "ih_m", "ho_m", "hidden", "output", "o_error"]


def elem(a, b, floor):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    big = np.abs(b) >= floor * max(np.abs(b).max(), 1e-300)
    return float((np.abs(a - b)[big] / np.abs(b)[big]).max()) if big.any() else 0.0


print("%-18s %-9s %9s %9s | element-wise, floor 1e-1 %9s 1e-2 %9s 1e-3" % ("shape H/S/D", "array", "2-norm", "max elem", "", ""))
# (the last two: the hot regime of the golden case hot_clamps and of the direct-delta-path test -- learn rate 0.08,
# streams soft-clipped, chains ending early: the error grows through the chain's steps)
SHAPES = ((99, 4, 10, 1e-3, 14), (256, 16, 8, 1e-4, 10), (1024, 8, 20, 1e-5, 22), (39, 4, 12, 0.08, 2), (128, 32, 8, 0.08, 2))
if len(sys.argv) > 1:
    SHAPES = [tuple(float(x) if "." in x or "e" in x else int(x) for x in arg.split(",")) for arg in sys.argv[1:]]
for (H, S, D, lr, warm, *more) in SHAPES:
    kw = dict(input_size=42, hidden_size=H, output_size=42, S=S, D=D, learn_rate=lr, seed=11)
    if more:  # activation, variance of the initial weights, seed
        kw.update(zip(("activation", "variance", "seed"), more))
    if lr == 0.08:
        warm = 2
    a = sc.ApiSet(strict, softmax_best_guess=strict.ref_softmax_best_guess, **kw)
    b = sc.ApiSet(fast, softmax_best_guess=fast.ref_softmax_best_guess, **kw)
    worst = {k: [0.0] * 5 for k in KEYS}
    for i in range(warm + (38 if lr == 0.08 else 3)):
        a.char_step(text, i, rc.WEIGHTED, 0.9)
        b.char_step(text, i, rc.WEIGHTED, 0.9)
        sa, sb = a.snapshot(), b.snapshot()
        if i >= warm:  # the ring is full: a generation at full depth, one generation deep from identical state
            for k in KEYS:
                v = [rc.rel_err(sb[k], sa[k]), rc.max_err(sb[k], sa[k])] + [elem(sb[k], sa[k], f) for f in (1e-1, 1e-2, 1e-3)]
                worst[k] = [max(x, y) for x, y in zip(worst[k], v)]
        # re-synchronise: the -Ofast side continues from the strict side's state
        n0, m0 = a.net.contents, b.net.contents
        for name, n in (("ih_weights", a.I * a.H), ("ho_weights", a.H * a.O)):
            rc.view(getattr(m0, name), n)[:] = rc.view(getattr(n0, name), n)
        for name, n in (("ih_momentum", a.I * a.H), ("ho_momentum", a.H * a.O)):
            rc.view(getattr(m0.bptt.contents, name), n)[:] = rc.view(getattr(n0.bptt.contents, name), n)
        for j in range(S):
            x, y = a.nets[j].contents, b.nets[j].contents
            rc.view(y.bptt.contents.history, a.D * a.I)[:] = rc.view(x.bptt.contents.history, a.D * a.I)
            rc.view(y.hidden_layer, a.H)[:] = rc.view(x.hidden_layer, a.H)
            y.bptt.contents.min_error_factor = x.bptt.contents.min_error_factor
    for k in KEYS:
        print("%-18s %-9s %9.2e %9.2e | %30.2e %14.2e %14.2e" % ("%d/%d/%d" % (H, S, D) + ("/a%d" % more[0] if more else ""), k, *worst[k]))
    a.close()
    b.close()
