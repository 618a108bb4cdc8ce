"""The two kernels of DESIGN.md section 31 without a GPU: a cross-compile of detect.hip and match.hip to gfx950 assembly
with the flags of csrc/Makefile, in the manner of test_rolling_layout.py.

orb_describe_kernel<256>: no scratch, at most 70 VGPRs (the `.num_vgpr` of the kernel: what it had before), and the loop of
the staged-region path -- the one with eight ds_read_u8 that neither writes LDS nor loads from memory -- has at most 28 VALU
instructions (40 before; the model of section 31 gives 22) and no v_cndmask.
sort_matches_kernel: no scratch, at most 64 VGPRs, and the loops of the counting form's placement walk (the ones with
v_mbcnt / v_bfe_i32) hold no v_addc_co_u32; the rank form's loop is still there, for the problems of at most a wave."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import check_mfma_hazards as chk  # noqa: E402

CSRC = os.path.join(ROOT, "vo_single_camera_sos_amd", "csrc")


def _kernel(text, pattern):
    """The one kernel whose symbol matches `pattern` -> (code, num_vgpr, scratch bytes)."""
    syms = sorted(set(re.findall(r"^(_ZN\S*?%s\S*):" % pattern, text, re.M)))
    assert len(syms) == 1, syms
    sym = syms[0]
    body = text[text.index(sym + ":"):]
    body = body[:body.index(".end_amdhsa_kernel")]
    code = body[:body.index("s_endpgm")]
    scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1))
    vg = int(re.search(r"\.set %s\.num_vgpr, (\d+)" % re.escape(sym), text).group(1))
    return code, vg, scratch


def _loops(code):
    """{header label: [opcodes of every block of that loop, inner loops included]} from the compiler's loop annotations."""
    blocks, cur = [], None
    for ln in code.splitlines():
        m = re.match(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)(.*)$", ln)
        if m:
            cur = {"label": m.group(1), "notes": m.group(2), "ops": []}
            blocks.append(cur)
        elif cur is not None and re.match(r"^\s+;", ln):
            cur["notes"] += ln
        elif cur is not None:
            op = re.match(r"^\s+([a-z]\w+)", ln)
            if op:
                cur["ops"].append(op.group(1))
    loops = {}
    for b in blocks:
        heads = set(re.findall(r"(?:Header=|Parent Loop )(BB\d+_\d+)", b["notes"]))
        if "Loop Header" in b["notes"]:
            heads.add(b["label"])
        for h in heads:
            loops.setdefault(h, []).extend(b["ops"])
    return loops


def _valu(ops):
    return [o for o in ops if o.startswith("v_")]


@pytest.fixture(scope="module")
def hipcc():
    if not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")):
        pytest.skip("no hipcc")


@pytest.fixture(scope="module")
def describe256(hipcc):
    return _kernel(chk.compile_hip(os.path.join(CSRC, "detect.hip")), r"19orb_describe_kernelILi256EE")


@pytest.fixture(scope="module")
def sort_kernel(hipcc):
    return _kernel(chk.compile_hip(os.path.join(CSRC, "match.hip")), r"19sort_matches_kernelE")


def test_describe_registers(describe256):
    code, vg, scratch = describe256
    assert scratch == 0 and "scratch_" not in code
    assert vg <= 70, "%d VGPRs" % vg


def test_describe_region_loop(describe256):
    code, _, _ = describe256
    region = [ops for ops in _loops(code).values()
              if ops.count("ds_read_u8") == 8 and not any(o.startswith(("ds_write", "global_load", "flat_load")) for o in ops)]
    assert len(region) == 1, "%d loops look like the staged-region loop" % len(region)
    valu = _valu(region[0])
    print("staged-region loop: %d VALU instructions: %s" % (len(valu), " ".join(valu)))
    assert len(valu) <= 28, "%d VALU instructions in the staged-region loop" % len(valu)
    assert not any(o.startswith("v_cndmask") for o in valu)
    assert sum(o.startswith("v_cmp") for o in valu) == 4            # the four ballots
    assert not any(o.startswith(("v_add3", "v_lshl_add_u64", "v_readfirstlane", "v_rndne", "v_cvt")) for o in valu)


def test_describe_other_paths_store_without_a_select_chain(describe256):
    """The per-keypoint-patch loop and the global-memory loop of the same kernel share the store: no v_cndmask in them."""
    code, _, _ = describe256
    loops = _loops(code)
    patch = [ops for ops in loops.values() if ops.count("ds_read_u8") == 8 and any(o.startswith("ds_write") for o in ops)]
    glob = [ops for ops in loops.values() if sum(o in ("global_load_ubyte", "flat_load_ubyte") for o in ops) == 8]
    assert len(patch) == 1 and len(glob) == 1
    for ops in patch + glob:
        assert not any(o.startswith("v_cndmask") for o in ops)
        assert sum(o.startswith("global_store_dwordx4") for o in ops) == 2


def test_sort_registers(sort_kernel):
    code, vg, scratch = sort_kernel
    assert scratch == 0 and "scratch_" not in code
    assert vg <= 64, "%d VGPRs" % vg


def test_sort_counting_loops(sort_kernel):
    code, _, _ = sort_kernel
    loops = _loops(code)
    walk = [ops for ops in loops.values() if "v_mbcnt_lo_u32_b32" in ops or "v_bfe_i32" in ops]
    assert len(walk) == 2, "the chunk loop and the loop over the bits of the bin index"
    for ops in walk:
        assert "v_addc_co_u32" not in [re.sub(r"_e(32|64)$", "", o) for o in ops]
        print("counting form, a loop of %d VALU instructions" % len(_valu(ops)))
    bits = min(walk, key=len)
    assert len(_valu(bits)) <= 4 and "v_bfe_i32" in bits, bits       # per bit: field, ballot, one three-input op per half
    rank = [ops for ops in loops.values() if sum(o.startswith("v_cmp_lt_u32") for o in ops) >= 4 and "ds_read_b128" in ops]
    assert rank, "the rank form's loop is gone"
