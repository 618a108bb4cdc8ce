"""GPU: scripts/fuzz_parity.py for a fixed number of cases per stage -- randomly drawn sizes / parameters of the median,
the GFT / FAST / AGAST / ORB detectors, the Hamming matchers, the omni one-call batch and the RGB-D batch with every
detector through the C ABI against the CPU oracle, bit for bit (the tool exits non-zero on the first difference and prints
the case to replay), and every stage must have completed all its cases."""
import ast
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fuzz_parity_fixed_cases():
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "fuzz_parity.py"), "--cases", "25", "--minutes", "6", "--seed", "20261004"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    last = out.stdout.splitlines()[-1]
    assert "all identical" in last, out.stdout[-500:]
    # every stage ran all 25 of its cases (a refused draw or the time limit would leave one short)
    cases = ast.literal_eval(re.search(r"cases (\{.*?\}) flagged", last).group(1))
    import importlib.util
    spec = importlib.util.spec_from_file_location("fuzz_parity_module", os.path.join(ROOT, "scripts", "fuzz_parity.py"))
    fp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fp)
    assert set(cases) == set(fp.STAGES) and {"batch", "rgbd"} <= set(cases), cases
    assert all(n == 25 for n in cases.values()), cases
