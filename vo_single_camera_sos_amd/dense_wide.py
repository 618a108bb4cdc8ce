"""Dense omnistereo with 16 to 256 disparities (include/sosvo_dense_wide.h): the binding of the extension
header's entry point and its checked Python face.  As in dense_filter, the call is a function that takes the Context first,
not a method of it: the Context is the face of include/sosvo.h, and its calls are pinned to a committed recording
(tests/test_context_calls.py).  There is no CPU fallback: a library without the symbol raises."""
import torch

from . import _lib
from ._lib import SosvoError, c_i32, c_p
from .device import _check, _check_opt, _ptr

# name -> (restype, argtypes): every function of include/sosvo_dense_wide.h
SIGNATURES = {
    "sosvo_dense_stereo_wide": (c_i32, [c_p, c_p, c_p, c_i32, c_i32, c_i32, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32,
                                        c_p, c_p]),
}

# the test and measurement hook of csrc/dense_wide.hip, which no header declares: the same arguments, the new kernels at every D
HOOKS = {"sosvo_debug_dense_stereo_wide_kernels": SIGNATURES["sosvo_dense_stereo_wide"]}

_bound = None


def load():
    """libsosvo.so (what _lib.load() returns) with the argument types of this header's function set (once)."""
    global _bound
    if _bound is None:
        lib = _lib.load()
        for name, (restype, argtypes) in list(SIGNATURES.items()) + list(HOOKS.items()):
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise SosvoError("libsosvo.so does not export %s; rebuild it" % name)
            fn.restype = restype
            fn.argtypes = argtypes
        _bound = lib
    return _bound


def dense_stereo(ctx, top, bot, mask=None, *, options=None, disparities=64, paths=4, want_volume=False,
                 _entry="sosvo_dense_stereo_wide"):
    """sosvo_dense_stereo_wide: Context.dense_stereo with `disparities` D, a multiple of 16 in 16 .. 256 (the reference tuner's
    num_of_disparities), searched from options.min_disparity on: top, bot [n,rows,cols] u8 gray panoramas, mask [rows,cols] u8
    or None, options a DenseOptions (None: the defaults), paths 4 or 8 -> d16 [n,rows,cols] i16 (disparity in 1/16 row, -1 =
    invalid); with want_volume (d16, S [n,rows,cols,D] u16).  D = 64 gives Context.dense_stereo's launches and bytes.  A bad
    disparities, paths or options value raises ValueError before the call."""
    o = _lib.DenseOptions.of(options)
    disparities = _lib.dense_disparities(disparities, paths, o)
    _check(top, torch.uint8, "top", ndim=3)
    n, rows, cols = top.shape
    _check(bot, torch.uint8, "bot", (n, rows, cols))
    _check_opt(mask, torch.uint8, "mask", (rows, cols))
    d16 = torch.empty((n, rows, cols), dtype=torch.int16, device=top.device)
    S = torch.empty((n, rows, cols, disparities), dtype=torch.uint16, device=top.device) if want_volume else None
    ctx._call(getattr(load(), _entry), _ptr(top), _ptr(bot), n, rows, cols, _ptr(mask), o.min_disparity, disparities, o.P1, o.P2,
              o.uniqueness, o.lr_max, o.flags, paths, _ptr(d16), _ptr(S))
    return (d16, S) if want_volume else d16


def debug_dense_stereo_wide_kernels(ctx, top, bot, mask=None, **kw):
    """dense_stereo through the hook sosvo_debug_dense_stereo_wide_kernels: the kernels of csrc/dense_wide.hip at every D, 64
    included, where dense_stereo runs the existing ones.  For the tests and scripts/bench_dense_wide.py."""
    return dense_stereo(ctx, top, bot, mask, _entry="sosvo_debug_dense_stereo_wide_kernels", **kw)
