"""The four-columns-per-lane blur without a GPU.

1. csrc/rolling_layout.h -- the load offsets, byte selectors and owned columns that gauss7_wide_kernel takes from
   sosvo_blur_wide_layout -- compiled for the host and evaluated for cols 3 .. 600 and every strip.  Below
   SOSVO_BLUR_WIDE_MIN_COLS the launcher runs the one-column form and the layout is not used: there the test checks the
   threshold itself (it is 8, and the single reflection the layout applies would already be wrong at cols = 3).  From the
   threshold on: every load offset lies in [0, cols - 4], so that the four bytes of any row, the last one included, end
   inside the image's rows * cols bytes; every column is owned by exactly one (strip, lane, byte); and a numpy model of the
   kernel's row step built from those offsets and selectors (load, v_perm_b32, the neighbours' dwords with zeros beyond
   lanes 0 and 63, v_alignbyte_b32 windows, two v_dot4_u32_u8), followed by the vertical pass, equals oracle.gauss7.
2. A cross-compile of detect.hip to gfx950 assembly, in the manner of test_median_isa.py: the wide blur kernel has no
   scratch, uses v_dot4_u32_u8 and v_alignbyte_b32, and exchanges two dwords per row where the one-column form moves six;
   the two-columns-per-lane response kernel has no scratch, stays at or below 96 VGPRs (five waves per SIMD, and room
   beside the median's three workgroups per CU), exchanges lanes through DPP only, and reads two mask words with one
   8-byte load in its interior instantiation."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import check_mfma_hazards as chk  # noqa: E402

CSRC = os.path.join(ROOT, "vo_single_camera_sos_amd", "csrc")
SHIM = r"""
#include "rolling_layout.h"
int min_cols(void) { return SOSVO_BLUR_WIDE_MIN_COLS; }
int strip_w(void) { return SOSVO_BLUR_WIDE_STRIP_W; }
int strips(int cols) { return sosvo_blur_wide_strips(cols); }
int edge_strip(int cols, int strip) { return sosvo_blur_wide_edge_strip(cols, strip); }
void layout(int cols, int strip, int32_t* off, uint32_t* sel, uint32_t* own) {
  for (int l = 0; l < 64; ++l) {
    sosvo_blur_wide_lane r = sosvo_blur_wide_layout(cols, strip, l);
    off[l] = r.off; sel[l] = r.sel; own[l] = r.own;
  }
}
"""
W_LO, W_HI = (18, 34, 49, 54), (49, 34, 18, 0)


@pytest.fixture(scope="module")
def lay(tmp_path_factory):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler")
    d = tmp_path_factory.mktemp("rolling_layout")
    src, so = str(d / "shim.c"), str(d / "shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.check_call([cc, "-O1", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + CSRC, "-o", so, src])
    lib = ctypes.CDLL(so)
    p32 = np.ctypeslib.ndpointer(np.int32, flags="C"), np.ctypeslib.ndpointer(np.uint32, flags="C")
    lib.layout.argtypes = [ctypes.c_int, ctypes.c_int, p32[0], p32[1], p32[1]]
    lib.layout.restype = None

    def layout(cols, strip):
        off, sel, own = np.zeros(64, np.int32), np.zeros(64, np.uint32), np.zeros(64, np.uint32)
        lib.layout(cols, strip, off, sel, own)
        return off, sel, own
    lib.layout_np = layout
    return lib


def _row_sums(lib, img):
    """Horizontal sums of every row of img by the kernel's row step, all strips; returns (H [rows, cols], owners [cols])."""
    rows, cols = img.shape
    H = np.zeros((rows, cols), np.int64)
    owners = np.zeros(cols, np.int32)
    first_w = lib.strip_w()
    for strip in range(lib.strips(cols)):
        off, sel, own = lib.layout_np(cols, strip)
        assert off.min() >= 0 and off.max() <= cols - 4, "cols %d strip %d: a load leaves the row" % (cols, strip)
        idx = off[:, None] + np.arange(4)[None, :]                      # [64, 4] columns of each lane's dword
        D = img[:, idx]                                                # [rows, 64, 4] the loaded bytes
        selb = (sel[:, None] >> (8 * np.arange(4, dtype=np.uint32))[None, :]) & 0xFF
        assert selb.max() <= 3
        if not lib.edge_strip(cols, strip):                            # the interior instantiation skips the permute
            assert (off == strip * first_w - 3 + 4 * np.arange(64)).all() and (selb == np.arange(4)).all()
        C = np.take_along_axis(D, np.broadcast_to(selb[None].astype(np.int64), D.shape), axis=2).astype(np.int64)
        L = np.concatenate([np.zeros_like(C[:, :1]), C[:, :-1]], axis=1)  # wave_shr:1, lane 0 receives 0
        R = np.concatenate([C[:, 1:], np.zeros_like(C[:, :1])], axis=1)   # wave_shl:1, lane 63 receives 0
        LC, CR = np.concatenate([L, C], axis=2), np.concatenate([C, R], axis=2)  # bytes 0 .. 7, low first
        for j in range(4):
            lo, hi = LC[:, :, j + 1: j + 5], CR[:, :, j + 1: j + 5]    # v_alignbyte_b32 by j + 1 (j = 3: C and R themselves)
            h = (lo * W_LO).sum(axis=2) + (hi * W_HI).sum(axis=2)
            x = strip * first_w - 3 + 4 * np.arange(64) + j
            m = ((own >> j) & 1).astype(bool)
            assert ((x[m] >= 0) & (x[m] < cols)).all()
            H[:, x[m]] = h[:, m]
            owners[x[m]] += 1
    return H, owners


def _vertical(H):
    rows = H.shape[0]
    w = np.array([18, 34, 49, 54, 49, 34, 18], np.int64)
    out = np.zeros_like(H)
    for k in range(-3, 4):
        r = np.arange(rows) + k
        if rows > 1:
            for _ in range(8):
                r = np.where(r < 0, -r, r)
                r = np.where(r >= rows, 2 * (rows - 1) - r, r)
        else:
            r = np.zeros(rows, np.int64)
        out += w[k + 3] * H[r]
    return ((out + 32768) >> 16).astype(np.uint8)


def test_threshold_is_stated_and_at_least_eight(lay):
    assert lay.min_cols() == 8 and lay.strip_w() == 250


@pytest.mark.parametrize("lo,hi", [(3, 150), (150, 300), (300, 450), (450, 601)])
def test_layout_model_equals_the_oracle(lay, lo, hi):
    rng = np.random.default_rng(lo)
    for cols in range(lo, hi):
        if cols < lay.min_cols():
            continue  # the launcher's one-column form (tests/test_gpu_blur_wide.py runs cols 3 .. 12 on the device)
        img = rng.integers(0, 256, (4, cols), dtype=np.uint8)
        img[rng.integers(0, 5, img.shape) == 0] = 255
        img[3] = 255
        H, owners = _row_sums(lay, img)
        assert (owners == 1).all(), "cols %d: a column is owned %s times" % (cols, sorted(set(owners.tolist())))
        assert np.array_equal(_vertical(H), oracle.gauss7(img)), "cols %d" % cols


def test_layout_holds_down_to_four_columns(lay):
    """A single reflection reaches every needed column from cols = 4 on: the threshold of 8 leaves a margin."""
    rng = np.random.default_rng(4)
    for cols in range(4, 8):
        img = rng.integers(0, 256, (3, cols), dtype=np.uint8)
        H, owners = _row_sums(lay, img)
        assert (owners == 1).all() and np.array_equal(_vertical(H), oracle.gauss7(img))


# ---- the compiled kernel -------------------------------------------------------------------------------------------
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


@pytest.fixture(scope="module")
def detect_asm():
    if not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    return chk.compile_hip(os.path.join(CSRC, "detect.hip"))


def test_wide_blur_kernel_isa(detect_asm):
    ops, vg, scratch, code = _kernel(detect_asm, "gauss7_wide_kernel")
    assert scratch == 0 and "scratch_" not in code
    assert vg <= 96, "%d VGPRs" % vg
    # two instantiations (interior, border) of seven unrolled row steps: 8 dot products and 6 byte windows per step
    assert ops.count("v_dot4_u32_u8") == 2 * 7 * 8
    assert ops.count("v_alignbyte_b32") == 2 * 7 * 6
    # lane exchanges: two per row step, against six in the one-column form
    assert sum(1 for ln in code.splitlines() if "wave_sh" in ln) == 2 * 7 * 2
    assert "ds_bpermute_b32" not in ops


def test_narrow_blur_kernel_is_still_there(detect_asm):
    ops, vg, scratch, code = _kernel(detect_asm, "gauss7_kernel")
    assert scratch == 0 and "v_dot4_u32_u8" not in ops


def test_wide_response_kernel_isa(detect_asm):
    ops, vg, scratch, code = _kernel(detect_asm, "min_eigen_wide_kernel")
    assert scratch == 0 and "scratch_" not in code
    assert vg <= 96, "%d VGPRs" % vg
    # the row loop exchanges by DPP in the border instantiation too: the only cross-lane reads through the LDS crossbar are
    # the epilogue's two wave reductions of the per-mask maxima (a broadcast and six shuffle steps each)
    assert ops.count("ds_bpermute_b32") <= 14 and "ds_swizzle_b32" not in ops
    assert sum(1 for ln in code.splitlines() if "wave_sh" in ln) >= 2 * 3 * 10
    assert ops.count("global_load_dwordx2") >= 3                             # the interior's mask words, two per load
    assert ops.count("v_sqrt_f32_e32") == 2 * 3 * 2                          # two instantiations, three row steps, two pixels
    assert "global_load_ubyte" not in ops and "global_load_ushort" not in ops  # no load that needs an extension at the load


def test_narrow_response_kernel_is_still_there(detect_asm):
    ops, vg, scratch, code = _kernel(detect_asm, "min_eigen_kernel")
    assert scratch == 0 and ops.count("v_sqrt_f32_e32") == 2 * 3
