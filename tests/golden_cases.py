"""Scenario definitions shared by tests/golden/make_golden.py (which runs them on
the REAL reference, oracle/_ref/librecur_ref.so, in the build container) and by
the tests (which replay them on the oracle restatement and on librecur_amd.so
and compare with the stored reference results).

Each scenario is a dict of plain parameters; ``run_scenario`` drives any driver
object with the ApiSet / OracleSet interface of scenarios.py.
"""
import os

import numpy as np

import recur_ctypes as rc

TEXT_LEN = 6000

# name -> parameters.  "steps" generations of the multi-tap text loop
# (charmodel-predict.c:288-311) from a freshly initialised net.
TRAIN_CASES = {
    "relu_weighted": dict(hidden=39, S=4, D=8, act=rc.RELU, method=rc.WEIGHTED, lr=1e-2, steps=30, seed=3),
    "relu_nesterov": dict(hidden=39, S=4, D=8, act=rc.RELU, method=rc.NESTEROV, lr=1e-2, steps=30, seed=3),
    "relu_adagrad": dict(hidden=39, S=4, D=8, act=rc.RELU, method=rc.ADAGRAD, lr=1e-2, steps=30, seed=3,
                         ballast=0.1),
    "resqrt_weighted": dict(hidden=39, S=4, D=8, act=rc.RESQRT, method=rc.WEIGHTED, lr=1e-2, steps=30, seed=4),
    "reclip_simplified": dict(hidden=39, S=4, D=8, act=rc.RECLIP20, method=rc.SIMPLIFIED_NESTEROV, lr=1e-2,
                              steps=30, seed=5),
    "relu_classical": dict(hidden=39, S=3, D=5, act=rc.RELU, method=rc.CLASSICAL, lr=3e-3, steps=20, seed=6),
    "relu_adadelta": dict(hidden=39, S=3, D=5, act=rc.RELU, method=rc.ADADELTA, lr=1e-3, steps=20, seed=7,
                          aux=True, momentum=0.95, ballast=0.0),
    "relu_rprop": dict(hidden=39, S=3, D=5, act=rc.RELU, method=rc.RPROP, lr=1e-3, steps=20, seed=8, aux=True,
                       aux_value=1e-4),
    # one generation only: a single forward/backward/update from a known state (G3)
    "single_step_h99": dict(hidden=99, S=3, D=10, act=rc.RESQRT, method=rc.WEIGHTED, lr=1e-3, steps=1, seed=9),
    "ragged_s7_h130": dict(hidden=130, S=7, D=6, act=rc.RELU, method=rc.WEIGHTED, lr=1e-3, steps=8, seed=10),
    # a learn rate high enough that the error-gain clamp (ih_scale < 1) and the
    # adaptive early exit both fire (recur-nn.c:387-413)
    "hot_clamps": dict(hidden=39, S=4, D=12, act=rc.RELU, method=rc.WEIGHTED, lr=0.08, steps=40, seed=11),
    # presynaptic noise: every stream draws from its own Jenkins generator
    # (recur-nn.c:120-121), so the final generator states are part of the parity
    "noisy": dict(hidden=39, S=4, D=6, act=rc.RELU, method=rc.WEIGHTED, lr=1e-2, steps=12, seed=15,
                  noise=0.05),
    # a bottom layer under the net (text-predict --bottom-layer): 42 symbols -> 16
    # rectified nodes -> 39 hidden.  bottom->o_error is never cleared on this path, so
    # the bottom deltas integrate every earlier stream and generation (recur-nn.c:377-382)
    "bottom_weighted": dict(hidden=39, S=4, D=8, act=rc.RELU, method=rc.WEIGHTED, lr=1e-2, steps=20,
                            seed=16, bottom=16, bottom_rate_scale=0.5),
    "bottom_adagrad_noisy": dict(hidden=39, S=3, D=6, act=rc.RESQRT, method=rc.ADAGRAD, lr=1e-2, steps=12,
                                 seed=17, bottom=12, ballast=0.1, noise=0.03),
    # ... and a bottom layer in the hot regime: a stream whose error gain is clipped shrinks the layer's
    # (shared, never cleared) error accumulator by ih_scale twice (recur-nn.c:391-399)
    "bottom_hot_clamps": dict(hidden=39, S=4, D=8, act=rc.RELU, method=rc.WEIGHTED, lr=0.05, steps=30,
                              seed=18, bottom=16, bottom_rate_scale=0.5),
    "depth1": dict(hidden=23, S=2, D=1, act=rc.RELU, method=rc.WEIGHTED, lr=1e-2, steps=6, seed=12),
}


def case_kwargs(c):
    flags = rc.FLAG_STANDARD | rc.FLAG_ADAPTIVE_MIN_ERROR
    if c.get("aux"):
        flags |= rc.FLAG_AUX_ARRAYS
    kw = dict(input_size=42, hidden_size=c["hidden"], output_size=42, S=c["S"], D=c["D"],
              activation=c["act"], learn_rate=c["lr"], seed=c["seed"], flags=flags,
              noise=c.get("noise", 0.0))
    if c.get("bottom"):
        kw.update(input_size=c["bottom"], bottom_inputs=42,
                  bottom_rate_scale=c.get("bottom_rate_scale", 1.0))
    return kw


from recur_amd.drivers import synthetic_text_np  # noqa: E402,F401


def prepare(driver, c, set_momentum_values, set_aux_values):
    """Optimiser ballast that some methods need before the first step."""
    if "ballast" in c and c["ballast"]:
        set_momentum_values(c["ballast"])
    if "aux_value" in c:
        set_aux_values(c["aux_value"])
        set_momentum_values(0.0)


def run_scenario(driver, c, text, trace=None):
    m = c.get("momentum", 0.9)
    for i in range(c["steps"]):
        driver.char_step(text, i, c["method"], m)
        if trace is not None:
            trace(i)


# ---- what the tests that used to call the compiled reference live compare against (tests/golden/ref_live.npz and
# ref_header_offsets.txt, written by tests/golden/make_golden_live.py where the reference is built)

LIVE_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_live.npz")
HEADER_OFFSETS_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_header_offsets.txt")

# tests/test_oracle_vs_ref.py: 25 generations from the same cold start, per activation and optimiser
RUN_KW = dict(input_size=42, hidden_size=57, output_size=42, S=5, D=9, learn_rate=5e-3, seed=17)
RUN_TEXT_LEN, RUN_GENERATIONS, RUN_MOMENTUM = 3000, 25, 0.9
RUN_ACTS = {"relu": rc.RELU, "resqrt": rc.RESQRT, "reclip20": rc.RECLIP20}
RUN_METHODS = {"weighted": rc.WEIGHTED, "nesterov": rc.NESTEROV}

# tests/test_gpu_parity.py: the hundred generations at full size on erewhon.txt (training entropy per window)
HUNDRED_KW = dict(input_size=42, hidden_size=1024, output_size=42, S=256, D=20, learn_rate=1e-6, seed=3)
HUNDRED_WINDOW, HUNDRED_GENERATIONS, HUNDRED_MOMENTUM = 25, 100, 0.9

# tests/test_gpu_parity.py: tools/pernet_rate.c's arguments (its printed mean error)
PERNET_ARGS = (("-H", "99", "-t", "1", "-d", "30", "-s", "400"), ("-H", "99", "-t", "3", "-d", "30", "-s", "150"),
               ("-H", "256", "-t", "2", "-d", "12", "-s", "60"))

# tests/test_abi.py: every field of every public struct and every enum value of recur-nn.h
STRUCT_FIELDS = {
    "RecurNN": ["i_size", "h_size", "o_size", "input_size", "hidden_size", "output_size", "ih_size",
                "ho_size", "flags", "log", "mem", "input_layer", "hidden_layer", "output_layer",
                "ih_weights", "ho_weights", "real_inputs", "rng", "bptt", "bottom_layer", "metadata",
                "generation", "presynaptic_noise", "activation"],
    "RecurNNBPTT": ["depth", "index", "i_error", "h_error", "o_error", "ih_momentum", "ho_momentum",
                    "history", "ih_delta", "ho_delta", "ih_delta_tmp", "ih_aux", "ho_aux", "mem",
                    "learn_rate", "ih_scale", "ho_scale", "momentum", "momentum_weight",
                    "min_error_factor"],
    "RecurExtraLayer": ["mem", "weights", "momentums", "aux", "delta", "inputs", "outputs", "i_error",
                        "o_error", "learn_rate_scale", "input_size", "output_size", "i_size", "o_size",
                        "overlap"],
    "struct RecurInitialisationParameters": [
        "method", "submethod", "bias_uses_submethod", "inputs_use_submethod", "fan_in_sum",
        "fan_in_step", "fan_in_min", "fan_in_ratio", "flat_variance", "flat_shape", "flat_perforation",
        "run_input_probability", "run_input_magnitude", "run_gain", "run_len_mean", "run_len_stddev",
        "run_n", "run_loop", "run_crossing_paths", "run_inputs_miss", "run_input_at_start"],
    "RecurErrorRange": ["start", "len"],
}
ENUMS = ["RNN_NET_FLAG_OWN_BPTT", "RNN_NET_FLAG_OWN_WEIGHTS", "RNN_NET_FLAG_LOG_APPEND",
         "RNN_NET_FLAG_LOG_HIDDEN_SUM", "RNN_NET_FLAG_LOG_WEIGHT_SUM",
         "RNN_NET_FLAG_BPTT_ADAPTIVE_MIN_ERROR", "RNN_NET_FLAG_NO_MOMENTUMS", "RNN_NET_FLAG_NO_DELTAS",
         "RNN_NET_FLAG_BOTTOM_LAYER", "RNN_NET_FLAG_AUX_ARRAYS", "RNN_COND_USE_SCALE", "RNN_COND_USE_ZERO",
         "RNN_COND_USE_LAWN_MOWER", "RNN_COND_USE_TALL_POPPY", "RNN_COND_USE_RAND",
         "RNN_NET_FLAG_STANDARD", "RNN_MOMENTUM_WEIGHTED", "RNN_MOMENTUM_NESTEROV",
         "RNN_MOMENTUM_SIMPLIFIED_NESTEROV", "RNN_MOMENTUM_CLASSICAL", "RNN_ADAGRAD", "RNN_ADADELTA",
         "RNN_RPROP", "RNN_LAST_LEARNING_METHOD", "RNN_INIT_ZERO", "RNN_INIT_FLAT", "RNN_INIT_FAN_IN",
         "RNN_INIT_RUNS", "RNN_RELU", "RNN_RESQRT", "RNN_RECLIP20", "RNN_INIT_DIST_UNIFORM",
         "RNN_INIT_DIST_GAUSSIAN", "RNN_INIT_DIST_LOG_NORMAL", "RNN_INIT_DIST_SEMICIRCLE",
         "RNN_CONDITIONING_INTERVAL", "RNN_COND_USE_OFFSET"]


def header_offsets(tmp_dir, include_dir):
    """One C program that prints the size and offset of every field in STRUCT_FIELDS, every enum value in ENUMS and
    the header's constants, compiled against the recur-nn.h in include_dir: its output."""
    import subprocess
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "recur-nn.h"', 'int main(void){']
    for st, fields in STRUCT_FIELDS.items():
        lines.append('printf("sizeof %s %%zu\\n", sizeof(%s));' % (st, st))
        for f in fields:
            lines.append('printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));'
                         % (st, f, st, f, st, f))
    for e in ENUMS:
        lines.append('printf("%s %%ld\\n", (long)%s);' % (e, e))
    lines.append('printf("%g %g %g %g\\n", (double)MAX_TOP_ERROR_FACTOR, (double)BASE_MIN_ERROR_FACTOR, '
                 '(double)WEIGHT_SCALE, (double)RNN_MOMENTUM_WEIGHT);')
    lines.append("return 0;}")
    src = os.path.join(str(tmp_dir), "offsets.c")
    exe = os.path.join(str(tmp_dir), "offsets")
    with open(src, "w") as f:
        f.write("\n".join(lines))
    subprocess.run(["gcc", "-std=gnu11", "-D_GNU_SOURCE", "-fcommon", "-w", "-I", include_dir, src, "-o", exe],
                   check=True)
    return subprocess.run([exe], capture_output=True, text=True, check=True).stdout
