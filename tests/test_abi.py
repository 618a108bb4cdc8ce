"""CPU: the C-ABI library loads and exports every symbol include/sosvo.h declares; the Python
signature table covers exactly that set.  No compute call is made here."""
import ctypes
import os

import pytest

from vo_single_camera_sos_amd import _lib


def test_library_is_built():
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"


def test_every_declared_symbol_is_exported_and_bound():
    declared = _lib.declared_functions()
    assert declared, "header parse found nothing"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), "libsosvo.so lacks %s" % name
    assert sorted(_lib.SIGNATURES) == declared


def test_abi_version_and_loud_failure_without_gpu():
    lib = _lib.load()
    assert lib.sosvo_abi_version() >= 1
    import torch
    if not torch.cuda.is_available():
        from vo_single_camera_sos_amd.device import Context
        with pytest.raises(_lib.SosvoError):
            Context(0)


_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_ROOT, "vo_single_camera_sos_amd", "csrc")
# the solver, trig and BRIEF-table headers that exist ONCE, under csrc/, and that the oracle's build reads from there
_SHARED_HEADERS = ("trig_core.h", "ransac_core.h", "epnp_core.h", "gp3p_core.h", "relpose_core.h", "orb_bit_pattern_31.h")


def test_no_header_name_exists_in_both_oracle_and_csrc():
    """A quoted #include resolves next to the including file first: a header in oracle/ with the name of one in csrc/
    would shadow the shared text in the oracle's build without any error."""
    def headers(d):
        return {f for f in os.listdir(d) if f.endswith(".h")}
    assert set(_SHARED_HEADERS) <= headers(_CSRC)
    both = headers(os.path.join(_ROOT, "oracle")) & headers(_CSRC)
    assert not both, "in oracle/ and in csrc/: %s" % sorted(both)


def test_oracle_build_reads_the_shared_headers_from_csrc():
    """One text, and both builds read it: the preprocessor's dependency list of the oracle's sources, taken with the
    oracle Makefile's own flags (`make deps` = $(CC) $(CFLAGS) -MM), names csrc/'s copy of every shared header and no
    other file called *_core.h.  (The device build includes them by quoted name from csrc/ itself.)"""
    import subprocess
    out = subprocess.check_output(["make", "-s", "--no-print-directory", "-C", os.path.join(_ROOT, "oracle"), "deps"], text=True)
    deps = {os.path.realpath(w) for w in out.split() if w.endswith(".h")}
    shared = {os.path.realpath(os.path.join(_CSRC, h)) for h in _SHARED_HEADERS}
    assert shared <= deps, "not read by the oracle's build: %s" % sorted(shared - deps)
    cores = {d for d in deps if d.endswith("_core.h")}
    assert cores <= shared, "other *_core.h files in the oracle's build: %s" % sorted(cores - shared)


def test_opencv_pattern_headers_and_c_entry_carry_the_data_file():
    """data/orb_bit_pattern_31.txt (OpenCV's bit_pattern_31_) == the generated header (one, under csrc/) == what the C ABI
    hands out (sosvo_orb_bit_pattern_31: host memory, no context, no GPU) == what the oracle hands out
    (orc_orb_pattern_opencv, compiled from the same header)."""
    import ctypes
    import importlib.util
    import os
    import numpy as np
    from vo_single_camera_sos_amd import _lib, orb_pattern
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gen_orb_pattern", os.path.join(root, "scripts", "gen_orb_pattern.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.main(check=True), "run python scripts/gen_orb_pattern.py"
    buf = np.zeros((512, 2), dtype=np.int8)
    assert _lib.load().sosvo_orb_bit_pattern_31(ctypes.c_void_p(buf.ctypes.data)) == 0
    assert np.array_equal(buf, orb_pattern.opencv_pattern())
    assert _lib.load().sosvo_orb_bit_pattern_31(None) != 0
    import oracle
    assert np.array_equal(oracle.orb_pattern(), orb_pattern.opencv_pattern())


def test_signatures_agree_with_the_header_by_kind():
    """Every prototype of include/sosvo.h against _lib.SIGNATURES, parameter by parameter: an int32_t / double / float /
    uint64_t / int64_t / size_t parameter or return type is the ctypes type of that name, and every pointer is c_void_p,
    c_char_p or a ctypes POINTER."""
    from sosvo_header import prototypes
    scalar = {"int32_t": ctypes.c_int32, "double": ctypes.c_double, "float": ctypes.c_float, "uint64_t": ctypes.c_uint64,
              "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t}

    def agrees(c_type, ct):
        if "*" in c_type:
            return ct in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(ct, ctypes._Pointer)
        return scalar[c_type.replace("const ", "")] is ct

    protos = prototypes()
    assert sorted(protos) == sorted(_lib.SIGNATURES) and len(protos) >= 100
    for entry, (ret, params) in protos.items():
        restype, argtypes = _lib.SIGNATURES[entry]
        assert agrees(ret, restype), "%s returns %s, bound as %s" % (entry, ret, restype)
        assert len(params) == len(argtypes), entry
        for (c_type, name), ct in zip(params, argtypes):
            assert agrees(c_type, ct), "%s: %s %s is bound as %s" % (entry, c_type, name, ct)
