"""Build-time guard on the median kernel's instruction budget: median_gray_kernel<11, true>, the
11-row unrolled body, priced per row with the measured per-opcode issue rates of scripts/isa_mix.py, stays at least 6 %
below the 582-instruction body it replaced (21361.6 priced cycles per 11 rows), at <= 128 VGPRs (four waves per SIMD; the
shared-device hint's three workgroups per CU assume it) and without scratch.  The K = 5 / 3 and plain forms keep no
scratch either.  No GPU needed: hipcc cross-compiles to assembly."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import check_mfma_hazards as chk  # noqa: E402
import isa_mix  # noqa: E402

HIPCC = "/opt/rocm/bin/hipcc"
ROWS = 11                       # the row loop is unrolled K = 11 times: the static body is 11 rows
MAIN_PRICED = 21361.6           # the layout with straddling slots and the subtract / minimum rank counter: 6403 VALU


def _kernel(text, k, fused):
    syms = sorted(set(re.findall(r"^(_ZN\S*median_gray_kernelILi%dELb%dE\S*):" % (k, int(fused)), text, re.M)))
    assert len(syms) == 1, syms
    body = text[text.index(syms[0] + ":"):]
    body = body[:body.index(".end_amdhsa_kernel")]
    code = body[:body.index("s_endpgm")]
    valu = [(m.group(1), ln) for ln in code.splitlines() for m in [re.match(r"^\s+(v_\w+)", ln)] if m]
    priced = sum(isa_mix.op_cycles(op, ln) for op, ln in valu)
    vg = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", body).group(1))
    scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1))
    return valu, priced, vg, scratch, code


@pytest.fixture(scope="module")
def image_asm():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    return chk.compile_hip(os.path.join(ROOT, "vo_single_camera_sos_amd", "csrc", "image.hip"))


def test_median_11_fused_budget(image_asm):
    valu, priced, vg, scratch, code = _kernel(image_asm, 11, True)
    assert vg <= 128, "median kernel at %d VGPRs: fewer than four waves per SIMD" % vg
    assert scratch == 0 and "scratch_" not in code
    assert not any(op.startswith("v_mfma") for op, _ in valu)
    per_row = priced / ROWS
    assert per_row <= 0.94 * MAIN_PRICED / ROWS, "%.1f priced cycles per row (main: %.1f)" % (per_row, MAIN_PRICED / ROWS)
    ops = [op for op, _ in valu]
    # the parts the budget rests on, per row: the select core is untouched (4 popcounts per plane and channel), the
    # rank counter needs neither a subtraction nor a minimum, and no ring slot needs a slow-rate left shift
    assert ops.count("v_bcnt_u32_b32") == ROWS * 96
    assert ops.count("v_min_u16_e32") == 0 and ops.count("v_min_u16") == 0
    assert ops.count("v_cmp_lt_i16_sdwa") == ROWS * 24
    # one 64-bit shift per slice, plus the rare edge path's four byte realignments per row
    assert ops.count("v_lshlrev_b64") + ops.count("v_lshrrev_b64") <= ROWS * (24 + 4)
    assert ops.count("v_mul_lo_u32") <= 4 and ops.count("v_mad_u64_u32") <= 4 * ROWS  # (prologue; the rare edge path)


@pytest.mark.parametrize("k,fused", [(11, False), (5, True), (5, False), (3, True), (3, False)])
def test_median_other_forms_no_scratch(image_asm, k, fused):
    valu, priced, vg, scratch, code = _kernel(image_asm, k, fused)
    assert vg <= 128 and scratch == 0 and "scratch_" not in code
