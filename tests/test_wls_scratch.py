"""CPU: sosvo_dense_wls's scratch layout (csrc/dense_wls_scratch.h, the function dense_wls.hip calls), built by the host compiler
-- tests/dense_wls_scratch_check.cpp measures and places it at n = 2, rows = 3, cols = 5, clamped and cyclic, against offsets
worked out by hand from the sizes include/sosvo_dense_filter.h and DESIGN.md section 41 state, and checks the bytes per pixel at
the working size and at the narrowest cyclic map."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "vo_single_camera_sos_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_the_wls_layout_is_the_documented_one(tmp_path):
    exe = str(tmp_path / "dense_wls_scratch_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, "-o", exe,
                           os.path.join(HERE, "dense_wls_scratch_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
