"""Build-time check of what k_delta_direct's loops give the vector ALU (no GPU needed: hipcc cross-compiles).

An f32 MFMA occupies the SIMD's vector ALU, and the loop is 98 % matrix pipe: every vector-ALU instruction between the
MFMAs is pipe time (0.7 - 0.9 us per launch and instruction at hidden 1024 / 256 streams / depth 20, profiles/NOTES_r07.md).
The loop once held four of them per iteration that the result did not need -- three v_cndmask_b32 that picked the rest
piece's column group out of the error quad, and a fourth that hipcc made of the address generator's wrap compare -- and
was 5.2 us per launch slower for it.  What has to stay:
  * the all-ones loop issues NO vector-ALU instruction besides its MFMAs;
  * the coefficient loop issues exactly its multiplies (the four registers of the error quad and each piece's column
    group, per iteration of the ring) and nothing else;
  * per iteration of the ring: the two 16-byte operand loads, two dwords per piece, and the coefficient's dword."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
RING = 5


def loop_blocks(body):
    """the basic blocks of a function's assembly that hold MFMAs: lists of instruction mnemonics"""
    blocks, cur = [], []
    for line in body.split("\n"):
        code = line.split(";")[0].strip()
        if not code:
            continue
        if re.match(r"^\.LBB\d+_\d+:$", code):
            blocks.append(cur)
            cur = []
            continue
        cur.append(code.split()[0])
        if code.startswith("s_cbranch") or code.startswith("s_branch"):
            blocks.append(cur)
            cur = []
    blocks.append(cur)
    return [b for b in blocks if any(m.startswith("v_mfma") for m in b)]


@pytest.fixture(scope="module")
def microbench_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    asm = str(tmp_path_factory.mktemp("dd_valu") / "dd.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-I" + os.path.join(ROOT, "recur_amd", "csrc"),
                    os.path.join(ROOT, "tools", "delta_direct_microbench.hip"), "-S", "--cuda-device-only", "-o", asm],
                   check=True, capture_output=True)
    return open(asm).read()


@pytest.mark.parametrize("npw", (1, 2))
def test_delta_direct_loops_keep_the_vector_alu_for_the_mfmas(microbench_asm, npw):
    sym = "_Z14k_delta_directILi8ELi5ELi%dEEv6DdArgs:" % npw
    body = microbench_asm[microbench_asm.index(sym):]
    body = body[:body.index("s_endpgm")]
    loops = loop_blocks(body)
    assert len(loops) == 2, [len(b) for b in loops]
    seen = []
    for b in loops:
        assert sum(1 for m in b if m.startswith("v_mfma")) == RING * (16 + npw)
        valu = [m for m in b if m.startswith("v_") and not m.startswith("v_mfma")]
        coef = bool(valu)
        seen.append(coef)
        if coef:  # the rare launch: the error quad and each piece's column group times the stream's coefficient
            assert valu == ["v_mul_legacy_f32"] * (RING * (4 + npw)), valu
        assert b.count("global_load_dwordx4") == RING * 2
        assert b.count("global_load_dword") == RING * (2 * npw + (1 if coef else 0))
        assert not any(m.startswith("ds_") or m.startswith("buffer_") or m.startswith("scratch_") for m in b)
    assert sorted(seen) == [False, True]
