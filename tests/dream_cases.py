"""What tests/test_dream_rule.py and tests/test_gpu_dream_sequences.py share: the numpy float32 restatement of
recur_amd/csrc/dream_rule.h (badmaths.h:55-68, gstparrot.c:576), the oracle's generator asked through ctypes, and the
build of tests/dream_rule_harness.cpp.  numpy rounds every float32 operation once and fuses none, which is the rule."""
import ctypes as C
import os
import subprocess

import numpy as np

import recur_ctypes as rc

ROOT = rc.ROOT
CSRC = os.path.join(ROOT, "recur_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "dream_rule_harness.cpp")
ORACLE_DIR = os.path.join(ROOT, "oracle")
CXX = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
LINK = ["-L", ORACLE_DIR, "-l:liboracle.so", "-Wl,-rpath," + ORACLE_DIR]
F = np.float32
EXTREME = F(4.97)


def build_harness(directory, extra=()):
    rc.load_oracle()   # (builds oracle/liboracle.so where it is missing)
    exe = os.path.join(str(directory), "dream_rule_harness")
    subprocess.run(CXX + list(extra) + [SRC, "-o", exe] + LINK, check=True)
    return exe


def np_fraction(x, broken=None):
    """Lambert's continued fraction without the clamp, float32 operation by operation"""
    x = np.asarray(x, F)
    c1, c2 = (F(62370.0), F(17325.0)) if broken == "swapped coefficient" else (F(17325.0), F(62370.0))
    with np.errstate(all="ignore"):
        x2 = x * x
        a = x * (F(135135.0) + x2 * (c1 + x2 * (F(378.0) + x2)))
        b = F(135135.0) + x2 * (c2 + x2 * (F(3150.0) + x2 * F(28.0)))
        return (a / b).astype(F)


def np_tanh(x, broken=None):
    """dream_tanh, and its broken forms"""
    x = np.asarray(x, F)
    r = np_fraction(x, broken)
    with np.errstate(invalid="ignore"):
        lo, hi = (x < -EXTREME, x > EXTREME) if broken == "< for <=" else (x <= -EXTREME, x >= EXTREME)
    return np.where(lo, F(-1.0), np.where(hi, F(1.0), r)).astype(F)


def np_next(a, noise, g, broken=None):
    """dream_next, and its broken form"""
    a, g, noise = np.asarray(a, F), np.asarray(g, F), F(noise)
    with np.errstate(all="ignore"):
        if broken == "a + a * g":
            return (a + a * (noise * g)).astype(F)
        return (a * (F(1.0) + noise * g)).astype(F)


def same_floats(a, b):
    """bit for bit, any NaN being as good as another"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | nan))


def generator(seed):
    g = rc.OrcRng()
    rc.load_oracle().orc_init_rand64(C.byref(g), seed)
    return g


def words(g):
    return np.array([g.a, g.b, g.c, g.d], np.uint64)


def from_words(w):
    return rc.OrcRng(int(w[0]), int(w[1]), int(w[2]), int(w[3]))


def gaussians(g, n):
    """n values of orc_cheap_gaussian_noise from g, in order"""
    orc = rc.load_oracle()
    return np.array([orc.orc_cheap_gaussian_noise(C.byref(g)) for _ in range(n)], F)


def hexfloat(x):
    return float(F(x)).hex()


def harness_rows(exe, directory, noise, raw, rng):
    """one launch's work by the host harness: raw [rows][n] float32, rng [rows][4] uint64 -> (frame, next, rng)"""
    raw = np.ascontiguousarray(raw, F)
    rows, n = raw.shape
    paths = [os.path.join(str(directory), "dream_" + x) for x in ("raw", "rng", "out")]
    raw.tofile(paths[0])
    np.ascontiguousarray(rng, np.uint64).tofile(paths[1])
    r = subprocess.run([exe, "rows", hexfloat(noise), str(rows), str(n)] + paths, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    return (np.fromfile(paths[2] + ".frame", F).reshape(rows, n), np.fromfile(paths[2] + ".next", F).reshape(rows, n),
            np.fromfile(paths[2] + ".rng", np.uint64).reshape(rows, 4))
