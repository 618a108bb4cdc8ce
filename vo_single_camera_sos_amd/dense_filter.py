"""The WLS disparity filter (include/sosvo_dense_filter.h): the binding of the extension header's two
entry points and their checked Python face.  The calls are functions that take the Context first, not methods of it: the
Context is the face of include/sosvo.h, and its calls are pinned to a committed recording (tests/test_context_calls.py); an
extension with a header of its own keeps its table and its calls beside it.  There is no CPU fallback: a library without
the symbols raises."""
import ctypes

import torch

from . import _lib
from ._lib import SosvoError, WlsOptions, c_f64, c_i32, c_p
from .device import _check, _check_opt, _ptr

# name -> (restype, argtypes): every function of include/sosvo_dense_filter.h
SIGNATURES = {
    "sosvo_dense_confidence": (c_i32, [c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_p]),
    "sosvo_dense_wls": (c_i32, [c_p, c_p, c_p, c_p, c_p, c_i32, c_i32, c_i32, c_f64, c_p, c_i32, c_f64, c_i32, c_p, c_p]),
}

_bound = None
_tables = {}


def load():
    """libsosvo.so (what _lib.load() returns) with the argument types of this header's functions set (once)."""
    global _bound
    if _bound is None:
        lib = _lib.load()
        for name, (restype, argtypes) in SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise SosvoError("libsosvo.so does not export %s; rebuild it" % name)
            fn.restype = restype
            fn.argtypes = argtypes
        _bound = lib
    return _bound


def _options(options, what):
    o = WlsOptions.of(options)
    if o is None:
        raise ValueError("%s needs a WlsOptions: None means that the filter is off, and then there is no call" % what)
    return o


def weight_table(options):
    """The host table sosvo_dense_wls reads, one ctypes array per options value (made once: WlsOptions.weight_table)."""
    if options not in _tables:
        _tables[options] = (ctypes.c_double * 256)(*options.weight_table())
    return _tables[options]


def dense_confidence(ctx, d16, *, options):
    """sosvo_dense_confidence: d16 [n,rows,cols] i16, options a WlsOptions (or a dict of its fields; radius, roll_ppm and
    cyclic are read) -> conf [n,rows,cols] u8: 255 inside a smooth surface, towards 0 at a depth discontinuity, 0 where the
    pixel has no disparity."""
    o = _options(options, "dense_confidence")
    _check(d16, torch.int16, "d16", ndim=3)
    n, rows, cols = d16.shape
    conf = torch.empty((n, rows, cols), dtype=torch.uint8, device=d16.device)
    ctx._call(load().sosvo_dense_confidence, _ptr(d16), n, rows, cols, o.radius, o.roll_ppm, o.flags, _ptr(conf))
    return conf


def dense_wls(ctx, d16, guide, *, options, conf=None, mask=None, out=None, want_planes=False):
    """sosvo_dense_wls: d16 [n,rows,cols] i16, guide [n,rows,cols] u8 (the gray panoramas the maps belong to), options a
    WlsOptions (or a dict of its fields), conf [n,rows,cols] u8 or None (255 on every valid pixel), mask [rows,cols] u8 or
    None -> the filtered map in `out` (None: a new tensor; d16 itself: in place); with want_planes (map, planes
    [n,2,rows,cols] f64: the final numerator and denominator)."""
    o = _options(options, "dense_wls")
    _check(d16, torch.int16, "d16", ndim=3)
    n, rows, cols = d16.shape
    _check(guide, torch.uint8, "guide", (n, rows, cols))
    _check_opt(conf, torch.uint8, "conf", (n, rows, cols))
    _check_opt(mask, torch.uint8, "mask", (rows, cols))
    if out is None:
        out = torch.empty_like(d16)
    _check(out, torch.int16, "out", (n, rows, cols))
    planes = torch.empty((n, 2, rows, cols), dtype=torch.float64, device=d16.device) if want_planes else None
    ctx._call(load().sosvo_dense_wls, _ptr(d16), _ptr(guide), _ptr(conf), _ptr(mask), n, rows, cols, o.lam, weight_table(o), o.iters,
              o.min_weight, o.flags, _ptr(out), _ptr(planes))
    return (out, planes) if want_planes else out
