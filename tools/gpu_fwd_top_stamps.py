"""The text step's forward pass + top layer by the workgroups' own marks: the one launch (k_fwd_top) against forward +
boundary + top of the two launches (GPU box).  Build with `tools/mkabl.sh bnd -DBND_STAMPS` and run twice with
RECUR_AMD_LIB=build/dev/abl_bnd/librecur_amd.so: as it is, and with RECUR_AMD_FWD_TOP=0.  With a `tools/mkabl.sh ft
-DFT_STAMPS` library (k_fwd_top's five phase stamps and no others: -DPC_STAMPS turns every kernel's on, and the launch is
then not the one that ships) it prints workgroup (0, 0)'s phases of the one launch instead.  Arguments: streams, samples.

Marks are s_memrealtime (100 MHz, shared by all CUs) at every workgroup's first and last instruction, overwritten by every
launch: a sample is 60 generations back to back, a synchronisation, and the last generation's marks."""
import ctypes as C
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np
import recur_ctypes as rc, scenarios as sc

amd = rc.load_amd()
amd.rnn_amd_fwd_top_launches.restype = C.c_long
S = int(sys.argv[1]) if len(sys.argv) > 1 else 256
samples = int(sys.argv[2]) if len(sys.argv) > 2 else 10
text = sc.synthetic_text(60000)
g = sc.AmdBatchedSet(amd, input_size=42, hidden_size=1024, output_size=42, S=S, D=20, learn_rate=1e-5, seed=1)
g.load_text(text)


def marks(kind, n):
    f = getattr(amd, "ramd_bnd_%s_stamps" % kind, None)
    if f is None:
        return None
    buf = np.zeros((2, 1024), np.uint64)
    f(C.c_void_p(buf.ctypes.data))
    b = buf[:, :n].astype(np.int64)
    return dict(first_start=b[0].min(), last_start=b[0].max(), first_end=b[1].min(), last_end=b[1].max())


i = 0
for _ in range(300):
    amd.rnn_amd_set_char_step(g.handle, i, rc.WEIGHTED, 0.95)
    i += 1
amd.rnn_amd_synchronize()
one = amd.rnn_amd_fwd_top_launches() > 0
print("form: %s, %d streams" % ("one launch (k_fwd_top)" if one else "two launches (k_fwd_fused + k_text_top2)", S))
us = lambda a, b: (b - a) / 100.0
rows = []
phases = []
for _ in range(samples):
    for _ in range(60):
        amd.rnn_amd_set_char_step(g.handle, i, rc.WEIGHTED, 0.95)
        i += 1
    amd.rnn_amd_synchronize()
    fwd = marks("fwd", 256 if one else (S // 32) * 32)
    if fwd is not None:
        if one:
            rows.append((us(fwd["first_start"], fwd["last_end"]), us(fwd["first_start"], fwd["last_start"]),
                         us(fwd["first_start"], fwd["first_end"])))
        else:
            top = marks("top", S)
            rows.append((us(fwd["first_start"], top["last_end"]), us(fwd["first_start"], fwd["last_end"]),
                         us(fwd["last_end"], top["first_start"]), us(top["first_start"], top["last_end"])))
    if one and hasattr(amd, "ramd_fwd_top_stamps"):
        st = np.zeros(8, np.uint64)
        amd.ramd_fwd_top_stamps(C.c_void_p(st.ctypes.data))
        t = st.astype(np.int64)
        phases.append([us(t[0], t[k]) for k in (1, 2, 4, 5)])
if rows:
    r = np.array(rows)
    names = ("span", "last workgroup started", "first workgroup ended") if one else ("span", "forward", "boundary", "top")
    for k, name in enumerate(names):
        print("%-24s median %6.2f us   min %6.2f   max %6.2f" % (name, np.median(r[:, k]), r[:, k].min(), r[:, k].max()))
if phases:
    p = np.median(np.array(phases), axis=0)
    print("workgroup (0, 0), us from its first instruction: tile stored and drained %.2f, flag raised %.2f, "
          "row tile's flags seen %.2f, end %.2f" % tuple(p))
