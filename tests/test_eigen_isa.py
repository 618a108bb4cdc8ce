"""Build-time guard on min_eigen_wide_kernel's instruction mix, from a cross-compile of detect.hip
with the library's flags (scripts/check_mfma_hazards.compile_hip adds csrc/Makefile's FLAGS_detect).  No GPU needed.

The body holds six row steps (two edge forms x three phases) plus prologue and epilogue.  Before section 32 it had 1368
static VALU instructions, 283 of them v_mov_b32 (register copies, DPP lane moves not counted), 58 packed single-precision
operations and 88 VGPRs.  Reached: 1206 VALU, 85 v_mov_b32, no packed operation, 80 VGPRs (six workgroups per CU where 88
allow five); the steady path of a row step has no plain v_mov_b32 at all.  The bounds below are the reached values plus a few
instructions of compiler slack."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import check_mfma_hazards as chk  # noqa: E402

CSRC = os.path.join(ROOT, "vo_single_camera_sos_amd", "csrc")
PARENT_VALU, PARENT_MOV, PARENT_VGPR = 1368, 283, 88
REACHED_VALU, REACHED_MOV, REACHED_VGPR = 1206, 85, 80
SLACK = 8


@pytest.fixture(scope="module")
def detect_asm():
    if not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    return chk.compile_hip(os.path.join(CSRC, "detect.hip"))


def _kernel(text, name):
    syms = sorted(set(re.findall(r"^(_ZN\S*?%d%sE\S*):" % (len(name), name), text, re.M)))
    assert len(syms) == 1, syms
    body = text[text.index(syms[0] + ":"):]
    body = body[:body.index(".end_amdhsa_kernel")]
    code = body[:body.index("s_endpgm")]
    ops = [m.group(1) for ln in code.splitlines() for m in [re.match(r"^\s+([a-z]\w+)", ln)] if m]
    vg = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", body).group(1))
    scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1))
    return ops, vg, scratch, code


def test_library_compiles_detect_without_the_slp_vectoriser():
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^FLAGS_detect\s*:=\s*(.*)$", makefile, re.M)
    assert m and "-fno-slp-vectorize" in m.group(1).split()
    assert "-fno-slp-vectorize" in chk.file_flags(os.path.join(CSRC, "detect.hip"))   # the scripts compile it the same way


def test_wide_response_kernel_mix(detect_asm):
    ops, vg, scratch, code = _kernel(detect_asm, "min_eigen_wide_kernel")
    valu = [o for o in ops if o.startswith("v_")]
    mov = [o for o in valu if re.fullmatch(r"v_mov_b32(_e32|_e64)?", o)]
    pk = [o for o in valu if o.startswith("v_pk_")]
    print("min_eigen_wide_kernel: %d VALU, %d v_mov_b32, %d v_pk_*, %d VGPRs" % (len(valu), len(mov), len(pk), vg))
    assert not pk, pk
    assert scratch == 0 and "scratch_" not in code
    assert vg <= REACHED_VGPR < PARENT_VGPR, "%d VGPRs: fewer than six waves per SIMD" % vg
    assert len(mov) <= REACHED_MOV + SLACK < PARENT_MOV, "%d v_mov_b32" % len(mov)
    assert len(valu) <= REACHED_VALU + SLACK < PARENT_VALU, "%d VALU instructions" % len(valu)
    # what the counts rest on: the running maximum is one v_max_f32 per pixel and row step (the ordered key's v_max_u32 is
    # left in the epilogue's two wave reductions only), and the two square roots per step are still there
    assert ops.count("v_max_f32") + ops.count("v_max_f32_e32") == 2 * 3 * 2
    assert ops.count("v_max_u32_e32") <= 2 * 6
    assert ops.count("v_sqrt_f32_e32") == 2 * 3 * 2


def test_no_packed_single_precision_in_the_rolling_kernels(detect_asm):
    for name in ("min_eigen_kernel", "gauss7_wide_kernel", "gauss7_kernel"):
        ops, vg, scratch, code = _kernel(detect_asm, name)
        assert scratch == 0 and not [o for o in ops if o.startswith("v_pk_") and o.endswith("_f32")], name


def test_detect_kernels_pass_the_hazard_check(detect_asm):
    assert len(chk.kernels_in(detect_asm)) >= 12
    report, bad = chk.check_text(detect_asm)
    assert not bad, report
    assert not report, "a kernel of detect.hip uses MFMA now: %s" % sorted(report)
