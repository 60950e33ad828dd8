"""The sampler of the text models restated on the oracle, as tests/test_char_predict_gpu.py restates it for
rnn_char_confabulate (charmodel-predict.c:29-60, badmaths.h:71-156): orc_softmax, with a bias orc_softmax again of
p * bias + score, a float32 cumulative sum in index order, u = float32(orc_rand_double), the pick the first i with
u < c[i], a u at or beyond the total drawn again.  Shared by tests/test_sample_rule.py (the rule on the CPU) and
tests/test_gpu_sample_texts.py (the batched call on the device, teacher-forced)."""
import ctypes as C

import numpy as np

import recur_ctypes as rc

GREEDY_BIAS = 100.0
MAX_ATTEMPTS = 64
TOL = 1e-4   # the project's parity bar, applied to a cumulative probability (at most 1)


def seeded(orc, seed):
    g = rc.OrcRng()
    orc.orc_init_rand64(C.byref(g), int(seed))
    return g


def words(g):
    return (g.a, g.b, g.c, g.d)


def cumulative(orc, score, bias):
    """c[i]: the float32 running total of the biased distribution of a row of float32 scores"""
    score = np.ascontiguousarray(score, np.float32)
    n = len(score)
    p = np.zeros(n, np.float32)
    orc.orc_softmax(rc.fptr(p), rc.fptr(score), n)
    if bias:
        tmp = (p * np.float32(bias)).astype(np.float32)  # a multiplication, then an addition: never fused
        tmp = (tmp + score).astype(np.float32)
        orc.orc_softmax(rc.fptr(p), rc.fptr(tmp), n)
    return np.cumsum(p, dtype=np.float32)  # sequential, in float32


def greedy(score):
    score = np.asarray(score)
    return int(len(score) - 1 - np.argmax(score[::-1]))  # the last of equal maxima (">=")


def strict_pick(c, u):
    """the first i with u < c[i], or -1"""
    hit = np.nonzero(u < c)[0]
    return int(hit[0]) if len(hit) else -1


def uniform(orc, g):
    return np.float32(orc.orc_rand_double(C.byref(g)))


def draw(orc, g, c):
    """the rule's draw: (pick or -1 at the cap, the u of every attempt)"""
    us = []
    for _ in range(MAX_ATTEMPTS):
        us.append(uniform(orc, g))
        pick = strict_pick(c, us[-1])
        if pick >= 0:
            return pick, us
    return -1, us


def near(c, u, tol=TOL):
    """u lies within tol of a boundary between two symbols, or of the total"""
    return bool(np.any(np.abs(c.astype(np.float64) - float(u)) < tol))


def scores_of(o, k, hot, alen, head):
    """stream k of an OracleSet fed the one-hot of `hot`: the scores of one head of its output row"""
    ans = o.orc.orc_one_hot_opinion(o.z, k, int(hot), 0.0)
    return np.ctypeslib.as_array(ans, shape=(o.output_size,))[head * alen:(head + 1) * alen].copy()


def greedy_margin(score):
    """how far the best score is in front of the next one of ANOTHER index, relative to the scores' size"""
    best = greedy(score)
    rest = np.delete(np.asarray(score, np.float64), best)
    return (float(score[best]) - rest.max()) / max(1.0, float(np.abs(score).max()))


def free_run(o, k, first, seed, max_len, bias, stop=-1, alen=None, head=0):
    """the oracle on its own: stream k draws up to max_len symbols.  Returns (symbols, the steps at which a u lay within
    TOL of a boundary -- or the best score within TOL of the next --, the generator afterwards)."""
    alen = alen or o.output_size
    g = seeded(o.orc, seed)
    sym, out, close = int(first), [], []
    for t in range(max_len):
        score = scores_of(o, k, sym, alen, head)
        if bias >= GREEDY_BIAS:
            sym = greedy(score)
            if greedy_margin(score) < TOL:
                close.append(t)
        else:
            c = cumulative(o.orc, score, bias)
            sym, us = draw(o.orc, g, c)
            assert sym >= 0
            if any(near(c, u) for u in us):
                close.append(t)
        out.append(sym)
        if sym == stop:
            break
    return np.array(out, np.uint8), close, words(g)


class Replay:
    """What following a device's text with the oracle found: per step the strict pick, whether the device's pick was
    acceptable, and whether the step was close to a boundary."""

    def __init__(self):
        self.strict, self.close, self.rng = [], [], None

    def differing(self, got):
        return int(np.sum(np.asarray(self.strict) != np.asarray(got, int)[:len(self.strict)]))


def replay(o, k, first, seed, got, bias, alen=None, head=0, before_step=None):
    """Teacher-forced: stream k of the oracle is fed the symbols the DEVICE chose (`got`), and at every step the oracle's
    own distribution and draw say whether that choice was one the rule allows: c[s - 1] - TOL <= u < c[s] + TOL.  A u
    within TOL of the total may have been drawn again or not: both are followed.  Asserts that every pick is acceptable.
    before_step(t), if given, is called before the oracle's forward pass of step t."""
    alen = alen or o.output_size
    g = seeded(o.orc, seed)
    r = Replay()
    sym = int(first)
    for t, s in enumerate(int(x) for x in got):
        if before_step:
            before_step(t)
        score = scores_of(o, k, sym, alen, head)
        if bias >= GREEDY_BIAS:
            r.strict.append(greedy(score))
            scale = max(1.0, float(np.abs(score).max()))
            assert float(score[s]) >= float(score.max()) - TOL * scale, (k, t, s, r.strict[-1])
            if greedy_margin(score) < TOL:
                r.close.append(t)
        else:
            c = cumulative(o.orc, score, bias)
            c64 = c.astype(np.float64)
            close, strict = False, None
            for _ in range(MAX_ATTEMPTS):
                u = uniform(o.orc, g)
                close = close or near(c, u)
                if strict is None and strict_pick(c, u) >= 0:
                    strict = strict_pick(c, u)
                below = c64[s - 1] if s > 0 else -np.inf
                if below - TOL <= float(u) < c64[s] + TOL:
                    break  # the device's pick is one this u allows
                assert float(u) >= c64[-1] - TOL, ("text %d step %d: the device picked %d, the oracle's u %r lies in %d"
                                                   % (k, t, s, u, strict_pick(c, u)))
            else:
                raise AssertionError("text %d step %d: no draw of the oracle allows the device's pick %d" % (k, t, s))
            r.strict.append(strict if strict is not None else -1)
            if close:
                r.close.append(t)
        sym = s
    r.rng = words(g)
    return r
