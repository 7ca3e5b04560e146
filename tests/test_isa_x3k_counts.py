"""Instruction counts of the k-major fp32x3 sampler's step loop in the built libdmip.so (CPU only; the histogram of
scripts/isa_issue_model.py --hist).

The loop of x3k_sampler_kernel<3, 3, false, 0> is bound by the sum of its vector-issue costs (one wave per SIMD, in-order
issue), so an instruction that returns unnoticed is a slowdown. Required by the arithmetic: 2,400
MFMAs (3 products x 3 chain tiles x 16 output tiles x (1 + 8 + 8) k-steps + the output layer's), 1,536 exp / rcp of
the activations plus the normals' handful. Not required, and capped at what the build that introduced this test
shows: copies between the AGPR and VGPR files (the parent of that build had 612 reads + 68 writes = 680) and s_nop
statements (273 there). No scratch access inside the loop.

Layer 1 runs its MFMAs in the VGPR form from an asm statement (csrc/dmip_x3k.h mfma16_l1), which the compiler's hazard
recognizer does not see: the test also checks what the source relies on, that nothing but the fragment reads and
their waits sits between those MFMAs and that 12 wait states follow the last one.
"""
import os
import re
import sys

import pytest

from conftest import ROOT

HEADLINE = "x3k_sampler_kernelILi3ELi3ELb0ELi0E"
ACCVGPR_CAP = 440  # 428 reads + 12 writes
S_NOP_CAP = 186


@pytest.fixture(scope="module")
def model(dmip):
    if not os.path.exists(dmip._lib.LIB_PATH):
        pytest.skip("libdmip.so not built")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import isa_issue_model
    return isa_issue_model, dmip._lib.LIB_PATH


@pytest.fixture(scope="module")
def hist(model):
    m, lib = model
    h, nop_states, mfma_vgpr = m.histogram(m.kernel_lines(lib, HEADLINE))
    print(f"\n[x3k step loop] {sum(h.values())} instructions; accvgpr_read {h.get('v_accvgpr_read_b32', 0)}, "
          f"accvgpr_write {h.get('v_accvgpr_write_b32', 0)}, s_nop {h.get('s_nop', 0)} ({nop_states} wait states), "
          f"VGPR-form MFMAs {mfma_vgpr}")
    return m, h


def test_step_loop_mfmas(hist):
    _, h = hist
    assert sum(n for op, n in h.items() if op.startswith("v_mfma")) == 2400
    assert h.get("v_mfma_f32_16x16x32_f16", 0) == 2400


def test_step_loop_transcendentals(hist):
    m, h = hist
    assert h.get("v_exp_f32_e32", 0) == 768 and h.get("v_rcp_f32_e32", 0) == 768
    n = sum(c for op, c in h.items() if m.cost(op) == 8)
    assert 1536 <= n <= 1536 + 8, n  # + the two normal pairs' log, sqrt, sin, cos


def test_step_loop_has_no_scratch(hist):
    _, h = hist
    assert not {op: n for op, n in h.items() if op.startswith("scratch_")}


def test_step_loop_accvgpr_copies_capped(hist):
    _, h = hist
    n = h.get("v_accvgpr_read_b32", 0) + h.get("v_accvgpr_write_b32", 0) + h.get("v_accvgpr_mov_b32", 0)
    assert n <= ACCVGPR_CAP < 680, n


def test_step_loop_s_nop_capped(hist):
    _, h = hist
    assert h.get("s_nop", 0) <= S_NOP_CAP < 273, h.get("s_nop", 0)


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("nt", [2, 3])
@pytest.mark.parametrize("noise", [0, 1])
def test_layer1_vgpr_mfmas_stand_alone(model, d, nt, noise):
    m, lib = model
    loop = m.loop_lines(m.kernel_lines(lib, f"x3k_sampler_kernelILi{d}ELi{nt}ELb{noise}ELi0E"))
    ops = []
    for l in loop:
        mm = re.match(r"\s+([a-z_0-9]+)\s*(.*?)\s*(//.*)?$", l)
        if mm:
            ops.append((mm.group(1), mm.group(2)))
    vg = [i for i, (op, a) in enumerate(ops) if op.startswith("v_mfma") and a.startswith("v")]
    assert len(vg) == 16 * nt, len(vg)  # layer 1: one MFMA per output tile and chain tile
    between = {op for op, _ in ops[vg[0]:vg[-1] + 1]}
    assert between <= {"v_mfma_f32_16x16x32_f16", "ds_read_b128", "s_waitcnt", "s_nop"}, between
    states, i = 0, vg[-1] + 1
    while ops[i][0] == "s_nop":
        states += int(ops[i][1].split()[0], 0) + 1
        i += 1
    assert states >= 12, (states, ops[i])
