"""Build-time guard on where the median kernel's gray stores sit.  A row's byte is stored at the
top of the NEXT row step, after that step's wait for its source pixel and before its new loads, so that the store has a
whole row of the wave's work behind it when the following wait comes; stored at the end of its own row it was four VALU
instructions ahead of an `s_waitcnt vmcnt(0)` and every wave stalled once per row for the store's acknowledgement.

For the K = 11 fused and plain kernels: walk the row loop in program-text order (conditional branches fall through, the
unconditional branch that closes the loop is followed to the loop header) and count, from every `global_store_byte`, the
VALU instructions up to the next `s_waitcnt` with a vmcnt field.  At least 300 for each of the 11 stores of the unrolled
body -- more than half of a row's 537 instructions; the body it replaces had 4 -- exactly 11 byte stores inside the loop
and one after it (the flush of the last output row), <= 128 VGPRs, no scratch.  No GPU needed: hipcc cross-compiles to
assembly."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import check_mfma_hazards as chk  # noqa: E402

HIPCC = "/opt/rocm/bin/hipcc"
ROWS = 11
MIN_VALU_TO_WAIT = 300


@pytest.fixture(scope="module")
def image_asm():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    return chk.compile_hip(os.path.join(ROOT, "vo_single_camera_sos_amd", "csrc", "image.hip"))


def _kernel(text, k, fused):
    syms = sorted(set(re.findall(r"^(_ZN\S*median_gray_kernelILi%dELb%dE\S*):" % (k, int(fused)), text, re.M)))
    assert len(syms) == 1, syms
    body = text[text.index(syms[0] + ":"):]
    body = body[:body.index(".end_amdhsa_kernel")]
    vg = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", body).group(1))
    scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1))
    code = body[:body.index("s_endpgm")]
    lines = [ln.split(";")[0].rstrip() for ln in code.splitlines()]
    return [ln for ln in lines if ln.strip()], vg, scratch


def _store_to_wait(lines):
    """-> (VALU counts from each byte store inside the row loop to the next vmcnt wait, byte stores after the loop)."""
    labels = {m.group(1): i for i, ln in enumerate(lines) for m in [re.match(r"^(\.L\w+):", ln)] if m}
    # the row loop: the unconditional backward branch that spans the most text, and the label it goes to
    back = [(i - labels[m.group(1)], i, labels[m.group(1)]) for i, ln in enumerate(lines)
            for m in [re.match(r"^\s+s_branch\s+(\.L\w+)", ln)] if m and labels.get(m.group(1), i) < i]
    assert back, "no loop found"
    _, tail, head = max(back)
    stores = [i for i, ln in enumerate(lines) if re.match(r"^\s+global_store_byte\b", ln)]
    assert all(i > head for i in stores), "a byte store ahead of the row loop"
    counts = []
    for s in (i for i in stores if i < tail):
        i, n, steps = s + 1, 0, 0
        while True:
            steps += 1
            assert steps < 4 * len(lines), "no vmcnt wait after the store at line %d" % s
            ln = lines[i]
            if re.match(r"^\s+s_waitcnt\b.*\bvmcnt\(", ln):
                break
            if re.match(r"^\s+v_\w+", ln):
                n += 1
            i = head if i == tail else i + 1   # text order; the loop's closing branch goes back to its header
        counts.append(n)
    return counts, sum(1 for i in stores if i > tail)


@pytest.mark.parametrize("fused", [True, False])
def test_median_11_stores_a_row_ahead_of_the_next_wait(image_asm, fused):
    lines, vg, scratch = _kernel(image_asm, 11, fused)
    assert vg <= 128, "median kernel at %d VGPRs: fewer than four waves per SIMD" % vg
    assert scratch == 0 and not any("scratch_" in ln for ln in lines)
    counts, after = _store_to_wait(lines)
    print("fused=%s: VALU instructions from each gray store to the next vmcnt wait: %s; stores after the loop: %d"
          % (fused, counts, after))
    assert len(counts) == ROWS and after == 1, (len(counts), after)
    assert min(counts) >= MIN_VALU_TO_WAIT, counts
