"""CPU: csrc/scratch_carver.h, the one place where a stage's scratch is laid out, built by the host compiler --
tests/scratch_carver_check.cpp runs one layout over a null base (measuring) and over an arena (placing) and compares offsets,
totals, the 256-byte rounding, the empty take and the typed pointers; then sosvo_dense_stereo's layout (csrc/dense_scratch.h,
the function dense.hip calls) at n = 2, rows = 3, cols = 5 with and without S_out and the left-right check, against offsets
worked out by hand from the sizes include/sosvo.h and DESIGN.md section 37 state."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "vo_single_camera_sos_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_measuring_and_placing_agree_and_the_dense_layout_is_the_documented_one(tmp_path):
    exe = str(tmp_path / "scratch_carver_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, "-o", exe,
                           os.path.join(HERE, "scratch_carver_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
