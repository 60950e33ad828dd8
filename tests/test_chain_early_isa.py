"""Build-time check of k_chain_persist_early's machine code (no GPU needed: hipcc cross-compiles).

The early form of the one-launch BPTT chain (recur_amd/csrc/k_chain_persist.h, EARLY) issues the first K blocks of a
half-step's burst between the finish's two row stores and the `s_waitcnt vmcnt(0)` that waits for their acknowledgement; the
flag that the 32 consumers of those rows poll comes behind that wait.  hipcc is free to move MFMAs across an inline-asm
wait, and a flag in front of the drain would be silently wrong (consumers fetch rows that have not arrived), so the order
is checked in the assembly of every build, for the three activations' instantiations:
  * in each of the two unrolled half-steps: row store, row store, exactly 8 x EARLY v_mfma_f32_16x16x4_f32, the next
    `s_waitcnt vmcnt(0)`, then the flag's store -- no other store, wait for memory, barrier or LDS write in between, and
    no LDS operation that the block itself does not have (its one read-ahead per block);
  * the burst exists once: 2 x 128 MFMAs in all, as in k_chain_persist;
  * no scratch memory, no accumulators shuffled through AGPRs, and no more registers than k_chain_persist's 227 (the
    accumulators now live across the wait);
  * the two wait-state rules of tools/isa_lint_async_loads.py that hipcc does not apply inside inline asm."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
MFMA = "v_mfma_f32_16x16x4_f32"


@pytest.fixture(scope="module")
def chain_asm(tmp_path_factory):
    asm = str(tmp_path_factory.mktemp("chain_early") / "chain.s")
    src = os.path.join(ROOT, "recur_amd", "csrc")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-I" + src, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(src, "kernels_chain.hip"), "-S", "--cuda-device-only", "-o", asm],
                   check=True, capture_output=True)
    return asm


def early_blocks():
    """PC_EARLY as k_tiles.h has it: the K blocks the plan asks the launcher for"""
    text = open(os.path.join(ROOT, "recur_amd", "csrc", "k_tiles.h")).read()
    return int(re.search(r"#define PC_EARLY (\d+)", text).group(1))


def kernels(asm):
    """symbol -> instructions (comments and labels dropped) of every k_chain_persist_early instantiation"""
    text = open(asm).read().split("\n")
    out = {}
    for st, line in enumerate(text):
        if line.startswith("_Z21k_chain_persist_early") and line.split(";")[0].rstrip().endswith(":"):
            body = []
            for l in text[st + 1:]:
                ins = l.split(";")[0].strip()
                if ins and not ins.endswith(":") and not ins.startswith("."):
                    body.append(ins)
                if "s_endpgm" in l:
                    break
            out[line.split(":")[0]] = body
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_the_first_blocks_stand_between_the_row_stores_and_the_drain(chain_asm):
    e = early_blocks()
    assert 1 <= e < 16
    ks = kernels(chain_asm)
    assert sorted(s[len("_Z21k_chain_persist_early"):][:9] for s in ks) == ["ILi%dELi%dE" % (a, e) for a in (1, 2, 5)], list(ks)
    for sym, body in ks.items():
        # the row stores are the only places where two plain dword stores through an SGPR base follow one another
        plain = lambda i: body[i].startswith("global_store_dword ") and " off" not in body[i] and " sc" not in body[i]
        pairs = [i for i in range(len(body) - 1) if plain(i) and plain(i + 1)]
        assert len(pairs) == 2, (sym, pairs)  # the two unrolled half-steps
        for i in pairs:
            window, mfmas, j = [], 0, i + 2
            while body[j] != "s_waitcnt vmcnt(0)":
                window.append(body[j])
                mfmas += body[j].startswith(MFMA)
                j += 1
                assert j - i < 200, sym
            assert mfmas == 8 * e, (sym, mfmas)
            # besides the MFMAs: branches over the block (a half-step that multiplies nothing), its counted LDS waits,
            # its read-ahead -- one ds_read_b128 per block --, accumulators set to zero and scalar bookkeeping; nothing
            # that stores, waits for memory or meets the other waves
            for ins in window:
                op = ins.split()[0]
                zero = op == "v_mov_b32_e32" and ins.endswith(", 0")
                assert op == MFMA or op == "ds_read_b128" or zero or (op.startswith("s_") and op not in ("s_barrier", "s_sleep")), (sym, ins)
                assert not (op == "s_waitcnt" and "vmcnt" in ins), (sym, ins)
            assert sum(ins.startswith("ds_read_b128") for ins in window) == e, (sym, window)
            assert not any(ins.startswith(("s_load", "s_buffer_load")) for ins in window), (sym, window)
            # behind the drain: the flag, one plain dword store, before any further MFMA or barrier
            k = j + 1
            while not body[k].startswith("global_store_dword"):
                assert not body[k].startswith((MFMA, "s_barrier", "global_load")), (sym, body[k])
                k += 1
                assert k - j < 40, sym
            assert plain(k), (sym, body[k])
        assert sum(ins.startswith(MFMA) for ins in body) == 256, sym


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_no_scratch_no_agprs_no_more_registers_and_no_hazards(chain_asm):
    text = open(chain_asm).read()
    ks = kernels(chain_asm)
    assert len(ks) == 3
    for sym, body in ks.items():
        assert not any("scratch_" in ins or "v_accvgpr" in ins for ins in body), sym
        meta = text[text.index(".name:           " + sym):]
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1)) <= 227, sym
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_lint_async_loads.py"), chain_asm, sym, "--hazards-only"],
                           capture_output=True, text=True)
        assert r.returncode == 0 and " 0 problems" in r.stdout, sym + "\n" + r.stdout[-3000:]
