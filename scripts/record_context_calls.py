#!/usr/bin/env python
"""Record what every method of device.Context does, without a device: which checks it makes in which order, which entry
point of the C ABI it calls with which argument in which position, what a buffer it allocates holds before the call, and
the structure of what it returns -- or the exception it refuses the call with.

    python scripts/record_context_calls.py              # write tests/golden/context_calls_parent.json
    python scripts/record_context_calls.py --check      # compare with the committed file, exit 1 on a difference
    python scripts/record_context_calls.py --coverage   # the lines of device.py the sweep does not execute

tests/golden/context_calls_parent.json was written by this script from device.py as it stood BEFORE the buffer records
were folded into one description each; tests/test_context_calls.py holds every later device.py to it.

The recorder context (tests/test_match_step.py's, generalised): Context.__new__, `_lib` a namespace that maps every name of
_lib.SIGNATURES to itself (a str that can also be called, for the few entry points device.py calls directly), `_call`
records (entry, {parameter name of include/sosvo.h: decoded argument}).  An argument is decoded as
  * the caller's tensor it points to: the Python argument or `out[...]` / `frames[...]` key, matched by data_ptr ("name+N":
    N bytes into it);
  * "alloc#k": the k-th buffer the method made itself, listed under "allocs" as [kind, dtype, shape, fill] (the torch
    creation functions are wrapped as seen from device.py);
  * "NULL" (a null pointer) or "None" (Python's None, which ctypes passes as one);
  * a struct: its type and bytes (a hash beyond 32 bytes); a host array: its values.
_lib.gray_pyramid_bytes, a host call into the library, is stood in for by its arithmetic: libsosvo.so is never loaded.
device._check stays on: the wrapper logs (name, dtype, shape spec, ndim) and then runs the real function, with
torch.Tensor.is_cuda answering True for the host tensors, so that of two broken rules the first one speaks.

Cases: every public method with its optional outputs left out and supplied, every switch once, and the refusals: for every
check that reaches one of the caller's tensors, that tensor with a wrong dtype, a wrong size in each checked dimension (or
one dimension more where only ndim is checked), non-contiguous and replaced by a non-tensor; and one case per hand-written
raise.  A generated refusal that is a SosvoError with exactly the message _check has for the broken rule is not written out:
it is counted in the "by_rule" of the plain call it was derived from; every other outcome is a line of its own.

Coverage (--coverage, the standard library's trace module): the sweep executes every line of device.py except
  * Context.__init__, close, __del__ and the real _call -- they need the library and a device;
  * _check's `raise ... must live on the GPU` -- the residency branch, tested on the GPU (tests/test_gpu_mirror.py).
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys
from contextlib import contextmanager

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from sosvo_header import parameter_names  # noqa: E402

from vo_single_camera_sos_amd import _lib, device  # noqa: E402
from vo_single_camera_sos_amd.device import Context, GrayPyramid  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "context_calls_parent.json")

# what the entry points that device.py calls directly return
DIRECT = {"sosvo_orb_pyramid_pixels": lambda rows, cols: 2 * rows * cols + 7, "sosvo_profile_count": lambda h: 2,
          "sosvo_frame_pair_batch_workspace": lambda cfg: 4096, "sosvo_frame_pair_batch_streams_workspace": lambda cfg, n: 8192,
          "sosvo_rgbd_pair_batch_workspace": lambda cfg: 2048, "sosvo_sequence_workspace": lambda cfg, w, s: 12288,
          "sosvo_rgbd_sequence_workspace": lambda cfg, w, s: 6144}


def gray_pyramid_bytes(nimg, rows, cols, levels):
    """_lib.gray_pyramid_bytes without the library (the recorder never loads it): the halved levels back to back."""
    if not 1 <= levels <= 8:
        raise _lib.SosvoError("sosvo_gray_pyramid_bytes(%r, %r, %r, %r) -> SOSVO_ERR_ARG" % (nimg, rows, cols, levels))
    n = 0
    for _ in range(1, levels):
        rows, cols = (rows + 1) // 2, (cols + 1) // 2
        n += nimg * rows * cols
    return n


def _bytes(b):
    b = bytes(b)
    return b.hex() if len(b) <= 32 else "sha1:" + hashlib.sha1(b).hexdigest()[:16]


def _dtype(dt):
    return str(dt).replace("torch.", "")


class Entry(str):
    """An entry point's name that can be called: the direct calls of device.py are recorded like the others."""
    rec = None

    @property
    def __name__(self):
        return str(self)

    def __call__(self, *args):
        names = parameter_names(self, with_ctx=True)
        assert len(args) == len(names), self
        self.rec.calls.append([str(self), {n: self.rec.dec(a) for n, a in zip(names, args)}])
        return DIRECT[str(self)](*args)


class _Proxy(object):
    """A module as device.py sees it, with some functions replaced."""

    def __init__(self, module, **replaced):
        self.__dict__.update(replaced)
        self._module = module

    def __getattr__(self, name):
        return getattr(self._module, name)


class Recorder(object):
    def __init__(self):
        self.checks, self.calls, self.allocs = [], [], []
        self.tensors, self.host, self.keep, self.checked = [], {}, [], []
        self.named = {}     # address of a struct the caller passed -> its argument name

    # ---- what device.py sees in place of torch, ctypes and _check
    def torch_proxy(self):
        def made(kind, fill=None):
            def f(*args, **kwargs):
                t = getattr(torch, kind)(*args, **kwargs)
                value = args[1] if kind == "full" else t.tolist() if kind == "from_numpy" else fill
                self.allocs.append([kind, _dtype(t.dtype), list(t.shape), value])
                self.tensors.append(("alloc#%d" % (len(self.allocs) - 1), t))
                return t
            return f
        return _Proxy(torch, **{k: made(k) for k in ("zeros", "empty", "full", "zeros_like", "empty_like", "from_numpy")})

    def ctypes_proxy(self):
        def cast(obj, typ):
            target = obj.contents if hasattr(obj, "contents") else obj
            self.host[ctypes.addressof(target)] = target
            self.keep.append(obj)
            return ctypes.cast(obj, typ)
        return _Proxy(ctypes, cast=cast)

    def check(self, real):
        def _check(t, dtype, name, shape=None, ndim=None):
            self.checks.append([name, _dtype(dtype), None if shape is None else list(shape), ndim])
            self.checked.append(t)
            return real(t, dtype, name, shape, ndim)
        return _check

    # ---- decoding
    def name_of(self, t, exact_only=False):
        for name, u in self.tensors:
            if u is t:
                return name
        if exact_only or not t.numel():
            return None
        p = t.data_ptr()
        for name, u in self.tensors:
            if u.numel() and u.data_ptr() == p:
                return name
        for name, u in self.tensors:
            if u.numel() and u.data_ptr() <= p < u.data_ptr() + u.numel() * u.element_size():
                return "%s+%d" % (name, p - u.data_ptr())
        return None

    def ptr(self, v):
        if v is None:
            return "NULL"
        if v in self.host:
            o = self.host[v]
            if isinstance(o, ctypes.Array):
                return {"host": type(o)._type_.__name__, "values": list(o)}
            return {"struct": type(o).__name__, "arg": self.named.get(v), "bytes": _bytes(o)}
        for name, u in self.tensors:
            if u.numel() and u.data_ptr() == v:
                return name
        for name, u in self.tensors:
            if u.numel() and u.data_ptr() <= v < u.data_ptr() + u.numel() * u.element_size():
                return "%s+%d" % (name, v - u.data_ptr())
        return {"raw": v} if v < (1 << 20) else "unknown pointer"

    def dec(self, a):
        if a is None:
            return "None"
        if isinstance(a, str):
            return str(a)
        if isinstance(a, (bool, int, float)):
            return a if not isinstance(a, bool) else int(a)
        if isinstance(a, ctypes.c_void_p):
            return self.ptr(a.value)
        if type(a).__name__ == "CArgObject":     # ctypes.byref
            return {"byref": type(a._obj).__name__, "bytes": _bytes(a._obj)}
        if isinstance(a, ctypes.Array):
            return {"array": type(a)._type_.__name__, "len": len(a)}
        return {"unknown": type(a).__name__}

    def describe(self, v):
        if isinstance(v, torch.Tensor):
            name = self.name_of(v, exact_only=True)
            return name if name is not None else {"view": self.name_of(v), "shape": list(v.shape)}
        if isinstance(v, dict):
            return {k: self.describe(x) for k, x in v.items()}
        if isinstance(v, tuple):
            return {"tuple": [self.describe(x) for x in v]}
        if isinstance(v, list):
            return [self.describe(x) for x in v]
        if isinstance(v, GrayPyramid):
            return {"GrayPyramid": {k: self.describe(getattr(v, k)) for k in ("gray", "upper", "levels", "row_range", "cyclic")}}
        return v if v is None or isinstance(v, (bool, int, float, str)) else {"unknown": type(v).__name__}

    # ---- the library's side of a call
    def _call(self, entry, *args):
        names = parameter_names(entry)
        assert len(args) == len(names), entry
        self.calls.append([str(entry), {n: self.dec(a) for n, a in zip(names, args)}])
        if entry == "sosvo_detect_gft_candidates" and args[8].value is None:
            args[7][:] = [16, 2, 3, 4, 5, 6]            # strip_w, strips, nchunks, chunk_rows, wcap, regions
        elif entry == "sosvo_timer_elapsed_ms":
            args[0]._obj.value = 1.5
        elif entry == "sosvo_profile_get":
            args[1].value, args[3]._obj.value = b"kernel%d" % args[0], 0.25 * (args[0] + 1)
        elif entry.endswith("sequence_frame_counts"):
            out = self.host[args[-1].value]
            out[:] = [10 + i for i in range(len(out))]


def leaves(kwargs):
    """The caller's tensors and structs: [(path, object)], a path being (argument,) or (argument, key or index)."""
    out = []
    for k, v in kwargs.items():
        if isinstance(v, dict):
            out += [((k, kk), vv) for kk, vv in v.items()]
        elif isinstance(v, (tuple, list)):
            out += [((k, i), vv) for i, vv in enumerate(v)]
        elif isinstance(v, GrayPyramid):
            out += [((k, a), getattr(v, a)) for a in ("gray", "upper", "row_range")]
        else:
            out.append(((k,), v))
    return out


def path_name(path):
    return path[0] if len(path) == 1 else "%s[%r]" % path


def run(method, kwargs):
    """One call of Context.<method>(**kwargs) under the recorder -> (outcome, [(check index, path of the caller's tensor)])."""
    rec = Recorder()
    for path, v in leaves(kwargs):
        if isinstance(v, torch.Tensor):
            rec.tensors.append((path_name(path), v))
        elif isinstance(v, ctypes.Structure):
            rec.named[ctypes.addressof(v)] = path_name(path)
    c = Context.__new__(Context)
    Entry.rec = rec
    c._lib = _Proxy(object(), **{name: Entry(name) for name in _lib.SIGNATURES})
    c._h, c._call = None, rec._call      # (no handle: close() has nothing to destroy)
    saved = device.torch, device.ctypes, device._check, device._lib
    device.torch, device.ctypes, device._check = rec.torch_proxy(), rec.ctypes_proxy(), rec.check(device._check)
    device._lib = _Proxy(_lib, gray_pyramid_bytes=gray_pyramid_bytes)
    try:
        try:
            ret = EXTRA[method](**kwargs) if method in EXTRA else getattr(c, method)(**kwargs)
        finally:
            device.torch, device.ctypes, device._check, device._lib = saved
    except Exception as e:      # noqa: BLE001 -- the refusal IS the outcome
        return {"raises": [type(e).__name__, str(e)]}, []
    where = []
    for i, t in enumerate(rec.checked):
        for path, v in leaves(kwargs):
            if v is t:
                where.append((i, path))
                break
    return {"checks": rec.checks, "allocs": rec.allocs, "calls": rec.calls, "returns": rec.describe(ret)}, where


@contextmanager
def host_tensors_pass_for_resident():
    """torch.Tensor.is_cuda answers True: the only part of _check that is skipped."""
    torch.Tensor.is_cuda = property(lambda self: True)
    try:
        yield
    finally:
        del torch.Tensor.is_cuda


# ---- the cases ----------------------------------------------------------------------------------------------------------------
F, NM, CAP, OUT_CAP, CORR_CAP, NP, S, ROWS, COLS, H, W, K = 2, 3, 8, 16, 10, 2, 5, 12, 20, 9, 11, 7
NI, P = 2 * F, F * NM            # images of a stereo batch (view-major); buckets of one view
HALO = 2 * _lib.SEAM_HALO
u8, i8, i16, i32, i64, u32, f32, f64 = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64, torch.uint32,
                                        torch.float32, torch.float64)


def z(dt, *shape):
    return torch.zeros(shape, dtype=dt)


def rig():
    return device.make_rig((COLS, ROWS, 0.5, 3.0), (COLS, ROWS, 0.5, 2.0), (0, 0, 1), (0, 0, -1), 0.5, 70.0, f2f_max_hdiff=2.5)


def batch_cfg(**kw):
    c = _lib.BatchCfg(n_pairs=2, H=H, W=W, rows=ROWS, cols=COLS, nmask=NM, kp_cap=CAP, frame_cap=OUT_CAP)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def rgbd_cfg():
    return _lib.RgbdBatchCfg(n_pairs=2, rows=ROWS, cols=COLS, kp_cap=CAP, frame_cap=OUT_CAP)


def frame_record(cap=OUT_CAP):
    return dict(m_top=z(f32, F, cap, 2), m_bot=z(f32, F, cap, 2), d_top=z(u8, F, cap, 32), d_bot=z(u8, F, cap, 32),
                X=z(f64, F, cap, 3), b_top=z(f64, F, cap, 3), b_bot=z(f64, F, cap, 3), M=z(i32, F), n_cand=z(i32, F))


def rgbd_record(cap=OUT_CAP):
    return dict(m=z(f32, F, cap, 2), d=z(u8, F, cap, 32), X=z(f64, F, cap, 3), b=z(f64, F, cap, 3), M=z(i32, F))


def corr(n=NP, central=False):
    d = dict(f=z(f64, n, CORR_CAP, 3), p=z(f64, n, CORR_CAP, 3), cam=z(i32, n, CORR_CAP), q=z(i32, n, CORR_CAP),
             t=z(i32, n, CORR_CAP), n=z(i32, n), n_top=z(i32, n))
    if central:
        del d["cam"], d["n_top"]
    return d


def ransac_out(counts=False):
    d = dict(T=z(f64, NP, 3, 4), mask=z(u8, NP, S), idx=z(i32, NP, S), n_inliers=z(i32, NP), info=z(i32, NP, 4))
    if counts:
        d["counts"] = z(i32, NP, K)
    return d


def pyramid(levels=3, row_range=None, cyclic=False):
    n = gray_pyramid_bytes(NI, ROWS, COLS, levels)
    return GrayPyramid(z(u8, NI, ROWS, COLS), z(u8, n), levels, row_range, cyclic)


# what is no method of Context: GrayPyramid.level as the shapes of the views
EXTRA = {"GrayPyramid.level": lambda levels, l: list(pyramid(levels).level(l).shape)}


def CASES():
    """[(method, variant, builder of the keyword arguments)]: a fresh set of tensors per call."""
    C = []

    def case(method, variant, **kw):
        C.append((method, variant, kw))

    def both(method, outs, **kw):
        """The call with every optional output left out, then with them supplied (builders: values are thunks)."""
        case(method, "plain", **kw)
        case(method, "outputs", **dict(kw, **outs))

    T = lambda dt, *shape: (lambda: z(dt, *shape))      # noqa: E731 -- a thunk: built anew for every call
    # ---- plumbing
    for h in ("shared_device", "match_unsplit", "rolling_narrow", "score_fp64_only"):
        case("set_hint_" + h, "plain")
        case("set_hint_" + h, "off", on=False)
    case("set_lk_options", "plain")
    case("set_lk_options", "dict", lk=dict(half=7, levels=3, fb_max=1.5))
    case("set_lk_options", "refused", lk=dict(half=0))
    case("set_stereo_lk_options", "plain")
    case("set_stereo_lk_options", "dict", stereo_lk=dict(half=4, max_shift=2.0))
    from types import SimpleNamespace
    case("set_stream", "plain", stream=SimpleNamespace(cuda_stream=4242))
    for m in ("synchronize", "timer_start", "timer_stop", "timer_elapsed_ms", "debug_fill_scratch", "profile_enable",
              "profile_read", "frame_pair_batch_join"):
        case(m, "plain")
    case("debug_fill_scratch", "byte", byte=0x5A)
    case("profile_enable", "off", on=False)
    for l in range(3):
        case("GrayPyramid.level", "level-%d" % l, levels=3, l=l)
    # ---- unwrap, median, seam-free stages
    maps = dict(map_x=T(f32, 2, ROWS, COLS), map_y=T(f32, 2, ROWS, COLS))
    both("unwrap", dict(pano=T(u8, 2, F, ROWS, COLS, 3)), omni=T(u8, F, H, W, 3), masks=T(u8, 2, H, W), **maps)
    case("unwrap", "no-masks", omni=T(u8, F, H, W, 3), masks=None, **maps)
    for m in ("unwrap_prepare", "unwrap_prepare_seam_free"):
        case(m, "plain", masks=T(u8, 2, H, W), omni_shape=(H, W), **maps)
        case(m, "no-masks", masks=None, omni_shape=(H, W), **maps)
    both("mask_bits_seam_free", dict(out=T(u32, 2, ROWS, COLS + HALO)), mask_bits=T(u32, 2, ROWS, COLS))
    case("keypoints_unpad", "plain", kp=T(f32, P, CAP, 2), n=T(i32, P), period=COLS)
    both("gray_unpad", dict(out=T(u8, NI, ROWS, COLS), row_range=T(i32, 2, 2)), gray=T(u8, NI, ROWS, COLS + HALO), cols=COLS)
    both("unwrap_table", dict(pano=T(u8, 2, F, ROWS, COLS, 3)), omni=T(u8, F, H, W, 3), table=T(u32, 2, ROWS, COLS, 2))
    both("median_gray", dict(gray=T(u8, 2, F, ROWS, COLS)), img=T(u8, 2, F, ROWS, COLS, 3), ksize=5)
    case("median_gray", "not-bgr", img=T(u8, F, ROWS, COLS, 4), ksize=5)
    case("median_gray", "too-few-dims", img=T(u8, COLS, 3), ksize=5)
    case("gray_rows_needed", "plain", mask_bits=T(u32, 2, ROWS, COLS), nmask=NM, edge=31, pattern=T(i8, 512, 2), cos_a=0.5, sin_a=-0.5)
    both("unwrap_median_gray", dict(gray=T(u8, NI, ROWS, COLS)), omni=T(u8, F, H, W, 3), table=T(u32, 2, ROWS, COLS, 2), ksize=5)
    case("unwrap_median_gray", "row_range", omni=T(u8, F, H, W, 3), table=T(u32, 2, ROWS, COLS, 2), ksize=5, row_range=T(i32, 2, 2))
    # ---- detectors and descriptors
    det = dict(gray=T(u8, NI, ROWS, COLS), mask_bits=T(u32, 2, ROWS, COLS), images_per_maskset=2, nmask=NM, cap=CAP)
    triple = dict(kp=T(f32, NI * NM, CAP, 2), n=T(i32, NI * NM), status=T(i32, NI * NM))
    for m in ("detect_agast", "detect_fast", "detect_gft"):
        both(m, triple, **det)
        case(m, "too-few-mask-sets", **dict(det, images_per_maskset=1))
    case("detect_fast", "threshold", threshold=25, **det)
    case("detect_gft", "settings", quality=0.05, min_distance=7.0, max_corners=123, **det)
    dsc = dict(gray=T(u8, NI, ROWS, COLS), kp=T(f32, NI * NM, CAP, 2), n=T(i32, NI * NM), nmask=NM, pattern=T(i8, 512, 2),
               cos_a=0.5, sin_a=-0.5)
    both("describe_orb", dict(desc=T(u8, NI * NM, CAP, 32), row_range=T(i32, 2, 2), edge=15), **dsc)
    case("detect_gft_candidates", "plain", gray=T(u8, NI, ROWS, COLS), mask_bits=T(u32, 2, ROWS, COLS), images_per_maskset=2, nmask=NM)
    case("detect_gft_candidates", "too-few-mask-sets", gray=T(u8, NI, ROWS, COLS), mask_bits=T(u32, 2, ROWS, COLS),
         images_per_maskset=1, nmask=NM)
    g7 = dict(gray=T(u8, NI, ROWS, COLS), nimg=NI, rows=ROWS, cols=COLS)
    both("gauss7", dict(out=T(u8, NI * 300), img_stride=ROWS * COLS, out_stride=300, row_range=T(i32, 2, 2)), **g7)
    case("gauss7", "stride-below-image", **dict(g7, out_stride=ROWS * COLS - 1))
    case("gauss7", "no-rows", **dict(g7, rows=0))
    case("gauss7", "gray-too-short", **dict(g7, nimg=NI + 1))
    case("gauss7", "out-too-short", out=T(u8, NI * ROWS * COLS - 1), **g7)
    case("gauss7", "no-images", **dict(g7, nimg=0))
    sub = dict(gray=T(u8, NI, ROWS, COLS), kp=T(f32, NI * NM, CAP, 2), n=T(i32, NI * NM), nmask=NM)
    both("refine_subpix", dict(half=3, max_iter=4, eps=0.5, row_range=T(i32, 2, 2)), **sub)
    for m in ("gray_pyramid", "gray_pyramid_cyclic"):
        case(m, "plain", gray=T(u8, NI, ROWS, COLS), levels=3)
        case(m, "outputs", gray=T(u8, NI, ROWS, COLS), levels=3, row_range=T(i32, 2, 2), out=lambda: pyramid(3))
        case(m, "one-level", gray=T(u8, NI, ROWS, COLS), levels=1)
        case(m, "too-many-levels", gray=T(u8, NI, ROWS, COLS), levels=40)
    lk = dict(pyr=lambda: pyramid(3), prev_img=T(i32, NP), next_img=T(i32, NP), prev_pts=T(f32, NP, CAP, 2), n=T(i32, NP))
    lk_out = lambda k: (lambda: tuple([z(f32, NP, CAP, 2), z(u8, NP, CAP), z(f32, NP, CAP), z(f32, NP, CAP, 2)][:k]))  # noqa: E731
    case("track_lk", "plain", **lk)
    case("track_lk", "outputs", out=lk_out(3), **lk)
    case("track_lk", "settings", half=4, max_iter=5, eps=0.5, min_eig=0.25, **lk)
    case("track_lk", "next_pts", next_pts=T(f32, NP, CAP, 2), **lk)
    case("track_lk", "next_pts-outputs", next_pts=T(f32, NP, CAP, 2), out=lk_out(3), **lk)
    case("track_lk", "fb_max", fb_max=1.5, **lk)
    case("track_lk", "fb_max-outputs", fb_max=1.5, out=lk_out(4), **lk)
    case("track_lk", "fb_max-three-outputs", fb_max=1.5, out=lk_out(3), **lk)
    case("track_lk", "cyclic", cyclic=True, **lk)
    case("track_lk", "cyclic-pyramid", **dict(lk, pyr=lambda: pyramid(3, cyclic=True)))
    case("track_lk", "cyclic-off", cyclic=False, **dict(lk, pyr=lambda: pyramid(3, cyclic=True)))
    case("track_lk", "row_range-one-level", **dict(lk, pyr=lambda: pyramid(1, row_range=z(i32, 2, 2))))
    case("track_lk", "no-pyramid", **dict(lk, pyr=T(u8, NI, ROWS, COLS)))
    slk = dict(gray=T(u8, NI, ROWS, COLS), kp_top=T(f32, P, CAP, 2), n_top=T(i32, P), kp_bot=T(f32, P, CAP, 2), n_bot=T(i32, P),
               keys=T(u32, P, CAP, 1), nmask=NM)
    both("refine_stereo_lk", dict(status=T(u8, P, CAP), row_range=T(i32, 2, 2), stereo_min_disp=1.0, stereo_max_hdiff=2.5,
                                  stereo_lk=dict(half=4, max_shift=2.0)), **slk)
    case("refine_stereo_lk", "flat-keys", **dict(slk, keys=T(u32, P, CAP)))
    case("refine_stereo_lk", "keys-k2", **dict(slk, keys=T(u32, P, CAP, 2)))
    case("refine_stereo_lk", "odd-images", **dict(slk, gray=T(u8, NI + 1, ROWS, COLS)))
    case("refine_stereo_lk", "bad-options", stereo_lk=dict(half=0), **slk)
    for n in (1, 2):
        trk = dict(rig=rig, frames=frame_record, ref_frame=T(i32, n), trk_top=T(f32, n, OUT_CAP, 2), trk_bot=T(f32, n, OUT_CAP, 2),
                   st_top=T(u8, n, OUT_CAP), st_bot=T(u8, n, OUT_CAP), corr_cap=CORR_CAP)
        f2f = dict(rig=rig, frames=frame_record, ref_frame=T(i32, n), cur_frame=T(i32, n), keys_top=T(u32, n, OUT_CAP, 1),
                   order_top=T(i32, n, OUT_CAP), keys_bot=T(u32, n, OUT_CAP, 1), order_bot=T(i32, n, OUT_CAP), corr_cap=CORR_CAP)
        cen = dict(frames=rgbd_record, ref_frame=T(i32, n), cur_frame=T(i32, n), keys=T(u32, n, OUT_CAP, 1),
                   order=T(i32, n, OUT_CAP), corr_cap=CORR_CAP)
        if n == 1:
            case("f2f_assemble_tracked", "one-pair", **trk)
            case("f2f_assemble", "one-pair", **f2f)
            case("f2f_assemble_central", "one-pair", **cen)
            continue
        both("f2f_assemble_tracked", dict(out=lambda: corr()), **trk)
        case("f2f_assemble_tracked", "cyclic", cyclic=True, **trk)
        both("f2f_assemble", dict(out=lambda: corr()), **f2f)
        case("f2f_assemble", "cyclic", cyclic=True, **f2f)
        both("f2f_assemble_central", dict(out=lambda: corr(central=True), pct_good_matches=0.5, max_hdiff=2.5), **cen)
    # ---- ORB
    PYR = DIRECT["sosvo_orb_pyramid_pixels"](ROWS, COLS)
    case("orb_pyramid_pixels", "plain", rows=ROWS, cols=COLS)
    case("orb_mask_pyramid", "plain", mask_bits=T(u32, 2, ROWS, COLS), nmask=NM)
    orb = dict(gray=T(u8, NI, ROWS, COLS), mask_pyr=T(u32, 2, PYR), images_per_maskset=2, nmask=NM, nfeatures=50)
    both("detect_orb", dict(kp4=T(f32, NI * NM, CAP, 4), resp=T(f32, NI * NM, CAP), n=T(i32, NI * NM)), cap=CAP, **orb)
    case("detect_orb", "too-few-mask-sets", cap=CAP, **dict(orb, images_per_maskset=1))
    both("describe_orb_levels", dict(desc=T(u8, NI * NM, CAP, 32), kp_xy=T(f32, NI * NM, CAP, 2)), gray=T(u8, NI, ROWS, COLS),
         kp4=T(f32, NI * NM, CAP, 4), n=T(i32, NI * NM), nmask=NM, pattern=T(i8, 512, 2))
    both("detect_describe_orb", dict(kp_xy=T(f32, NI * NM, CAP, 2)), pattern=T(i8, 512, 2), kp4=T(f32, NI * NM, CAP, 4),
         resp=T(f32, NI * NM, CAP), n=T(i32, NI * NM), desc=T(u8, NI * NM, CAP, 32), **orb)
    # ---- matching: Bq = Bt = 3 blocks of Sq = 5 / St = 7 rows; with slots 4 problems over 3 / 6 blocks
    Sq, St = 5, 7
    mh = dict(q_desc=T(u8, 3, Sq, 32), t_desc=T(u8, 3, St, 32), nq=T(i32, 3), nt=T(i32, 3))
    pos = dict(q_pos=T(f32, 3, Sq, 2), t_pos=T(f32, 3, St, 2))
    slots = dict(mh, t_desc=T(u8, 6, St, 32), nt=T(i32, 6), q_slot=T(i32, 4), t_slot=T(i32, 4))
    spos = dict(pos, t_pos=T(f32, 6, St, 2))
    both("match_hamming", dict(keys=T(u32, 3, Sq, 2), k=2), **mh)
    both("match_hamming", dict(keys=T(u32, 4, Sq, 1)), **slots)
    case("match_hamming", "q_slot-alone", **dict(mh, q_slot=T(i32, 4)))
    case("match_hamming", "blocks-differ", **dict(slots, q_slot=None, t_slot=None))
    both("match_hamming_gated", dict(keys=T(u32, 3, Sq, 1), max_distance=80, n_forward=2), min_dv=1.0, max_du=2.5, **mh, **pos)
    case("match_hamming_gated", "slots", min_dv=1.0, max_du=2.5, n_forward=3, **slots, **spos)
    both("match_hamming_gated_cyclic", dict(keys=T(u32, 3, Sq, 1), max_distance=80, n_forward=2), max_du=2.5, period=COLS, **mh, **pos)
    case("match_hamming_gated_cyclic", "slots", max_du=2.5, period=COLS, **slots, **spos)
    both("match_hamming_ratio", dict(keys=T(u32, 3, Sq, 1), rivals=T(u32, 3, Sq, 1), n_forward=2), ratio_64ths=48, **mh)
    both("match_hamming_ratio", dict(keys=T(u32, 4, Sq, 1), rivals=T(u32, 4, Sq, 1), max_distance=80, n_forward=3, min_dv=1.0,
                                     max_du=2.5), ratio_64ths=48, **slots, **spos)
    case("match_hamming_ratio", "q_pos-alone", ratio_64ths=48, q_pos=T(f32, 3, Sq, 2), **mh)
    case("match_hamming_ratio", "cap-without-gate", ratio_64ths=48, max_distance=80, **mh)
    gate = (1.0, 2.5, 80)
    for name, kw in (("plain", {}), ("gate", dict(gate=gate, **pos)), ("gate-no-cap", dict(gate=(-1.0, 2.5, None), **pos)),
                     ("ratio", dict(ratio_64ths=48, rivals=T(u32, 3, Sq, 1))),
                     ("ratio-gate", dict(ratio_64ths=48, gate=gate, n_forward=2, **pos)),
                     ("period", dict(gate=(-1.0, 2.5, 80), period=float(COLS), n_forward=2, **pos)),
                     ("period-no-gate", dict(period=float(COLS))),
                     ("period-ratio", dict(gate=(-1.0, 2.5, 80), period=float(COLS), ratio_64ths=48, **pos)),
                     ("period-v-side", dict(gate=gate, period=float(COLS), **pos)),
                     ("outputs", dict(keys=T(u32, 3, Sq, 1)))):
        case("match_1nn", name, **mh, **kw)
    case("match_1nn", "slots", gate=gate, n_forward=3, **slots, **spos)
    blocks = dict(desc=T(u8, 6, Sq, 32), pos=T(f32, 6, Sq, 2), n=T(i32, 6))
    for name, nprob, kw in (("forward-only", 3, {}), ("cross-check", 6, {}), ("cross-check-gate", 6, dict(gate=gate)),
                            ("ratio", 6, dict(ratio_64ths=48, rivals=T(u32, 6, Sq, 1))),
                            ("period", 6, dict(gate=(-1.0, 2.5, None), period=float(COLS)))):
        case("match_1nn_slots", name, q_slot=T(i32, nprob), t_slot=T(i32, nprob), keys=T(u32, nprob, Sq, 1), n_forward=3, **blocks, **kw)
    for name, kw in (("plain", {}), ("cross_check", dict(cross_check=True)),
                     ("cross_check-outputs", dict(cross_check=True, keys=T(u32, 3, Sq, 1), keys_rev=T(u32, 3, St, 1))),
                     ("cross_check-gate-ratio", dict(cross_check=True, gate=gate, ratio_64ths=48, **pos)),
                     ("cross_check-period", dict(cross_check=True, gate=(-1.0, 2.5, None), period=float(COLS), **pos))):
        case("match_1nn_two_launch", name, **mh, **kw)
    case("match_l2", "plain", q_desc=T(f32, 3, Sq, 6), t_desc=T(f32, 3, St, 6), nq=T(i32, 3), nt=T(i32, 3))
    case("match_l2", "k", q_desc=T(f32, 3, Sq, 6), t_desc=T(f32, 3, St, 6), nq=T(i32, 3), nt=T(i32, 3), k=2)
    case("match_radius", "plain", max_distance=40, cap=4, **mh)
    case("match_radius", "slots", max_distance=40, cap=4, **slots)
    cc = dict(keys_fwd=T(u32, 3, Sq, 1), keys_rev=T(u32, 3, St, 1), nq=T(i32, 3), nt=T(i32, 3))
    both("cross_check_matches", dict(keys_out=T(u32, 3, Sq, 1), n_kept=T(i32, 3)), **cc)
    both("cross_check_matches", dict(keys_out=T(u32, 3, Sq, 1), n_kept=T(i32, 3)), q_slot=T(i32, 3), t_slot=T(i32, 3),
         **dict(cc, nq=T(i32, 6), nt=T(i32, 4)))
    case("cross_check_matches", "t_slot-alone", t_slot=T(i32, 3), **cc)
    case("cross_check_matches", "nq-per-block", **dict(cc, nq=T(i32, 6)))
    case("cross_check_matches", "nt-per-block", **dict(cc, nt=T(i32, 6)))
    both("sort_matches", dict(order=T(i32, 3, Sq)), keys=T(u32, 3, Sq, 1), nq=T(i32, 3))
    case("sort_matches", "q_slot", keys=T(u32, 3, Sq, 1), nq=T(i32, 6), q_slot=T(i32, 3))
    case("sort_matches", "nq-per-block", keys=T(u32, 3, Sq, 1), nq=T(i32, 6))
    # ---- pose
    ab = dict(f=T(f64, NP, S, 3), p=T(f64, NP, S, 3), n=T(i32, NP), thr=0.01, max_iter=K)
    cams = dict(cam=T(i32, NP, S), cam_off=T(f64, 2, 3), cam_rot=T(f64, 2, 3, 3))
    both("ransac_abs_pose", dict(out=lambda: ransac_out()), **ab)
    case("ransac_abs_pose", "want_counts", want_counts=True, seed=-3, adaptive=True, **ab)
    case("ransac_abs_pose", "counts-supplied", out=lambda: ransac_out(counts=True), **ab)
    case("ransac_abs_pose", "cam", cam_rot_identity=True, **ab, **cams)
    for s in ("epnp", "gp3p", "twopt"):
        case("ransac_abs_pose", s, **dict(ab, **{s: True}))
    case("ransac_abs_pose", "nine-cameras", **ab, **dict(cams, cam_off=T(f64, 9, 3), cam_rot=T(f64, 9, 3, 3)))
    case("ransac_abs_pose", "no-cameras", **ab, **dict(cams, cam_off=T(f64, 0, 3), cam_rot=T(f64, 0, 3, 3)))
    for m, extra in (("ransac_abs_pose", {}), ("ransac_abs_pose_seeds", dict(cam_rot_identity=True))):
        case(m, "seeds-host", seeds=[5, -1], **ab, **extra)
        case(m, "seeds-tensor", seeds=lambda: torch.tensor([5, 6], dtype=i64), out=lambda: ransac_out(), **ab, **extra)
        case(m, "seeds-too-few", seeds=[5], **ab)
        case(m, "seeds-int32", seeds=T(i32, NP), **ab)
        case(m, "seeds-strided", seeds=lambda: z(i64, 2 * NP)[::2], **ab)
    case("ransac_abs_pose_seeds", "no-seeds", seeds=None, **ab)
    rel = dict(f1=T(f64, NP, S, 3), f2=T(f64, NP, S, 3), n=T(i32, NP), thr=0.01, max_iter=K)
    case("ransac_rel_pose", "plain", **rel)
    case("ransac_rel_pose", "want_counts", want_counts=True, algorithm=_lib.REL_FIVEPT, seed=-3, adaptive=True, **rel)
    lm = dict(f=T(f64, NP, S, 3), p=T(f64, NP, S, 3), n=T(i32, NP), T=T(f64, NP, 3, 4))
    both("refine_abs_pose", dict(cost=T(f64, NP), iters=T(i32, NP), idx=T(i32, NP, S), m=T(i32, NP), max_lm_iter=9), **lm)
    case("refine_abs_pose", "cam", **lm, **cams)
    case("refine_abs_pose", "idx-alone", idx=T(i32, NP, S), **lm)
    # ---- geometry, dense, RGB-D
    case("pano_to_bearing", "plain", uv=T(f64, S, 2), cols=COLS, rows=ROWS, pixel_size=0.5, cyl_height_max=3.0)
    case("triangulate_midpoint", "plain", az_top=T(f64, S), el_top=T(f64, S), az_bot=T(f64, S), el_bot=T(f64, S),
         F_top=(0, 0, 1), F_bot=(0, 0.5, -1))
    case("triangulate2", "plain", b1=T(f64, S, 3), b2=T(f64, S, 3), t12=(1, 2, 3), R12=((1, 0, 0), (0, 0, -1), (0, 1, 0)))
    case("range_filter", "plain", X=T(f64, S, 3), min_range=0.5, max_range=70.0)
    case("census", "plain", gray=T(u8, NI, ROWS, COLS))
    case("census", "cyclic", gray=T(u8, NI, ROWS, COLS), cyclic=True)
    ds = dict(top=T(u8, F, ROWS, COLS), bot=T(u8, F, ROWS, COLS))
    case("dense_stereo", "plain", **ds)
    case("dense_stereo", "mask-options", mask=T(u8, ROWS, COLS), options=dict(P1=5, P2=50, cyclic=True), **ds)
    case("dense_stereo", "want_volume", want_volume=True, **ds)
    case("dense_stereo", "paths-8", paths=8, want_volume=True, **ds)
    case("dense_stereo", "paths-5", paths=5, **ds)
    case("dense_triangulate", "plain", rig=rig, d16=T(i16, F, ROWS, COLS))
    case("dense_triangulate", "gates", rig=rig, d16=T(i16, F, ROWS, COLS), min_disparity=1.3, max_disparity=40.2)
    case("dense_triangulate", "upper-gate-below-a-sixteenth", rig=rig, d16=T(i16, F, ROWS, COLS), max_disparity=0.01)
    sp = dict(d16=T(i16, F, ROWS, COLS), options=dict(max_size=9, max_diff=16))
    both("dense_speckle", dict(out=T(i16, F, ROWS, COLS)), **sp)
    case("dense_speckle", "want_labels", want_labels=True, **sp)
    case("dense_speckle", "no-options", d16=T(i16, F, ROWS, COLS), options=None)
    case("rgbd_backproject", "plain", depth=T(f32, ROWS, COLS), u=T(i32, S), v=T(i32, S), fx=525.0, fy=526.0, cx=9.5, cy=5.5,
         focal_length_m=0.001, depth_is_Z=True)
    both("stereo_assemble", dict(out=frame_record), rig=rig, kp_top=T(f32, P, CAP, 2), kp_bot=T(f32, P, CAP, 2),
         desc_top=T(u8, P, CAP, 32), desc_bot=T(u8, P, CAP, 32), n_top=T(i32, P), n_bot=T(i32, P), keys=T(u32, P, CAP, 1),
         order=T(i32, P, CAP), nframes=F, nmask=NM, out_cap=OUT_CAP)
    both("rgbd_assemble", dict(out=rgbd_record), cam=lambda: _lib.RgbdCam(fx=525.0, fy=526.0, cx=9.5, cy=5.5, max_range=4.0),
         kp=T(f32, F, CAP, 2), desc=T(u8, F, CAP, 32), n=T(i32, F), depth=T(f32, F, ROWS, COLS), out_cap=OUT_CAP)
    # ---- the one-call batches and sequence mode
    case("frame_pair_batch_workspace", "plain", cfg=batch_cfg)
    case("frame_pair_batch_streams_workspace", "plain", cfg=batch_cfg, n_streams=2)
    case("rgbd_pair_batch_workspace", "plain", cfg=rgbd_cfg)
    ws = T(u8, 4096)
    omni_consts = dict(unwrap_table=T(u32, 2, ROWS, COLS, 2), mask_bits=T(u32, 2, ROWS, COLS), pattern=T(i8, 512, 2), workspace=ws)
    fpb = dict(rig=rig, cfg=batch_cfg, omni=T(u8, 4, H, W, 3), **omni_consts)
    both("frame_pair_batch", dict(results=T(f64, 2, 16)), **fpb)
    case("frame_pair_batch", "streams-join", n_streams=2, **fpb)
    case("frame_pair_batch", "streams-enqueue", n_streams=2, join=False, **fpb)
    case("frame_pair_batch", "seam-free", **dict(fpb, cfg=lambda: batch_cfg(ransac_flags=_lib.FLAG_SEAM_FREE),
                                                 unwrap_table=T(u32, 2, ROWS, COLS + HALO, 2), mask_bits=T(u32, 2, ROWS, COLS + HALO)))
    rgbd_consts = dict(mask_bits=T(u32, 1, ROWS, COLS), pattern=T(i8, 512, 2), workspace=ws)
    both("rgbd_pair_batch", dict(results=T(f64, 2, 16)), cam=lambda: _lib.RgbdCam(fx=525.0), cfg=rgbd_cfg, bgr=T(u8, 4, ROWS, COLS, 3),
         depth=T(f32, 4, ROWS, COLS), **rgbd_consts)
    seq = dict(cfg=batch_cfg, window=3, slots=6)
    rseq = dict(cfg=rgbd_cfg, window=3, slots=6)
    rcam = lambda: _lib.RgbdCam(fx=525.0)     # noqa: E731
    case("sequence_workspace", "plain", **seq)
    case("rgbd_sequence_workspace", "plain", **rseq)
    case("sequence_front_end", "plain", rig=rig, omni=T(u8, 3, H, W, 3), first_slot=2, **seq, **omni_consts)
    case("sequence_front_end", "seam-free", rig=rig, omni=T(u8, 3, H, W, 3), first_slot=2,
         **dict(seq, cfg=lambda: batch_cfg(ransac_flags=_lib.FLAG_SEAM_FREE)),
         **dict(omni_consts, unwrap_table=T(u32, 2, ROWS, COLS + HALO, 2), mask_bits=T(u32, 2, ROWS, COLS + HALO)))
    case("sequence_front_end_slots", "plain", rig=rig, omni=T(u8, 3, H, W, 3), slot_of_frame=[4, 0, 2], **seq, **omni_consts)
    case("sequence_front_end_slots", "one-slot-short", rig=rig, omni=T(u8, 3, H, W, 3), slot_of_frame=[4, 0], **seq, **omni_consts)
    case("rgbd_sequence_front_end", "plain", cam=rcam, bgr=T(u8, 3, ROWS, COLS, 3), depth=T(f32, 3, ROWS, COLS), first_slot=2,
         **rseq, **rgbd_consts)
    case("rgbd_sequence_front_end_slots", "plain", cam=rcam, bgr=T(u8, 3, ROWS, COLS, 3), depth=T(f32, 3, ROWS, COLS),
         slot_of_frame=[4, 0, 2], **rseq, **rgbd_consts)
    case("rgbd_sequence_front_end_slots", "one-slot-short", cam=rcam, bgr=T(u8, 3, ROWS, COLS, 3), depth=T(f32, 3, ROWS, COLS),
         slot_of_frame=[4], **rseq, **rgbd_consts)
    for prefix, heads in (("sequence_", dict(rig=rig, **seq)), ("rgbd_sequence_", rseq)):
        trk = dict(ref_slots=[0, 1], cur_slots=[1, 2], workspace=ws, results=T(f64, 3, 16), **heads)
        case(prefix + "track", "plain", seed=-7, **trk)
        case(prefix + "track", "no-pairs", seed=1, **dict(trk, ref_slots=[], cur_slots=[]))
        case(prefix + "track", "lengths-differ", seed=1, **dict(trk, cur_slots=[1]))
        case(prefix + "track", "results-too-short", seed=1, **dict(trk, results=T(f64, 1, 16)))
        case(prefix + "track_seeds", "plain", seeds=[-1, 2 ** 63], **trk)
        case(prefix + "track_seeds", "seeds-differ", seeds=[1], **trk)
        case(prefix + "track_seeds", "slots-differ", seeds=[1, 2], **dict(trk, cur_slots=[1]))
        cp = dict(workspace=ws, **(seq if prefix == "sequence_" else rseq))
        case(prefix + "copy_slot", "plain", src=1, dst=4, **cp)
        case(prefix + "copy_slots", "plain", src_slots=[1, 2], dst_slots=[4, 5], **cp)
        case(prefix + "copy_slots", "lengths-differ", src_slots=[1, 2], dst_slots=[4], **cp)
        case(prefix + "frame_counts", "plain", first_slot=1, n=3, **cp)
        case(prefix + "frame_counts", "none", first_slot=1, n=0, **cp)
    return C


def build(kw):
    return {k: (v() if callable(v) else v) for k, v in kw.items()}


def _other_dtype(dt):
    return f64 if dt == f32 else f32


def _strided(t):
    """The same shape and dtype, not contiguous (None: every dimension is 1 or the tensor is empty)."""
    for d in reversed(range(t.dim())):
        if t.shape[d] > 1 and t.numel():
            shape = list(t.shape)
            shape[d] *= 2
            return torch.zeros(shape, dtype=t.dtype)[(slice(None),) * d + (slice(None, None, 2),)]
    return None


def _grown(t, d):
    shape = list(t.shape)
    shape[d] += 1
    return torch.zeros(shape, dtype=t.dtype)


def _replace(kwargs, path, value):
    if len(path) == 1:
        kwargs[path[0]] = value
        return
    box = kwargs[path[0]]
    if isinstance(box, dict):
        kwargs[path[0]] = dict(box, **{path[1]: value})
    elif isinstance(box, GrayPyramid):
        g = GrayPyramid(box.gray, box.upper, box.levels, box.row_range, box.cyclic)
        setattr(g, path[1], value)
        kwargs[path[0]] = g
    else:
        kwargs[path[0]] = tuple(value if i == path[1] else x for i, x in enumerate(box))


def _broken_rules(name, dtype, shape, ndim):
    """[(label, mutate(tensor), says(tensor))] for one check: says = the message _check has for the broken rule."""
    rules = [("dtype", lambda t: torch.zeros(t.shape, dtype=_other_dtype(t.dtype)),
              lambda t: "%s: dtype %s, expected torch.%s" % (name, _other_dtype(t.dtype), dtype)),
             ("strided", _strided, lambda t: "%s: must be contiguous" % name),
             ("no-tensor", lambda t: "no tensor", lambda t: "%s: expected a torch tensor, got <class 'str'>" % name)]
    rules += [("dim%d" % d, lambda t, d=d: _grown(t, d),
               lambda t, d=d: "%s: shape %s, expected %s" % (name, tuple(_grown(t, d).shape), tuple(shape)))
              for d, s in enumerate(shape or []) if s is not None]
    if ndim is not None:
        rules.append(("ndim", lambda t: t.unsqueeze(0), lambda t: "%s: ndim %d, expected %d" % (name, t.dim() + 1, ndim)))
    return rules


def refusals(method, kw, outcome, where, seen):
    """For every check of `outcome` that reached one of the caller's tensors: (label, path, mutate, says) per broken rule."""
    out = []
    for i, path in where:
        for label, change, says in _broken_rules(*outcome["checks"][i]):
            key = (method, path, outcome["checks"][i][0], label)
            if key not in seen:
                seen.add(key)
                out.append(("%s:%s" % (path_name(path), label), path, change, says))
    return out


def sweep():
    """Every case -> [{"id": ..., outcome}], in a fixed order.  A generated refusal that is a SosvoError with exactly the
    message _check has for the broken rule is counted in its plain call's "by_rule"; every other one is a record of its own."""
    records, seen, ids = [], set(), set()

    def unique(cid):
        while cid in ids:
            cid += "+"
        ids.add(cid)
        return cid
    with host_tensors_pass_for_resident():
        for method, variant, kw in CASES():
            outcome, where = run(method, build(kw))
            cid, extra = unique("%s/%s" % (method, variant)), 0
            records.append(dict(id=cid, **outcome))
            for label, path, change, says in refusals(method, kw, outcome, where, seen):
                kwargs = build(kw)
                box = kwargs[path[0]]
                leaf = box if len(path) == 1 else getattr(box, path[1]) if isinstance(box, GrayPyramid) else box[path[1]]
                new = change(leaf)
                if new is None:
                    continue
                _replace(kwargs, path, new)
                mid, refused = unique("%s!%s" % (cid, label)), run(method, kwargs)[0]
                if refused == {"raises": ["SosvoError", says(leaf)]}:
                    by_rule = records[-1 - extra]["by_rule"] = records[-1 - extra].get("by_rule", 0) + 1
                    assert by_rule
                else:
                    records.append(dict(id=mid, **refused))
                    extra += 1
    return records


def text(records):
    return "[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in records) + "\n]\n"


def uncovered_lines():
    """Lines of device.py that neither importing the module nor the sweep executes -> {line: enclosing function, as
    Class.name, or None}, by the standard library's trace module."""
    import ast
    import importlib.util
    import trace
    path = device.__file__

    def import_again():     # (under another name: what the `def`, `class` and constant statements execute)
        spec = importlib.util.spec_from_file_location(device.__package__ + "._device_traced", path)
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    tracer = trace.Trace(count=1, trace=0)
    tracer.runfunc(import_again)
    tracer.runfunc(sweep)
    hit = {line for (f, line), n in tracer.results().counts.items() if f == path and n}
    owner = {}

    def walk(node, prefix):
        for child in ast.iter_child_nodes(node):
            if isinstance(child, ast.ClassDef):
                walk(child, prefix + child.name + ".")
            elif isinstance(child, ast.FunctionDef):
                owner.update({line: prefix + child.name for line in range(child.lineno, child.end_lineno + 1)})
    walk(ast.parse(open(path).read()), "")
    return {line: owner.get(line) for line in sorted(set(trace._find_executable_linenos(path)) - hit)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--coverage", action="store_true")
    args = ap.parse_args()
    if args.coverage:
        src = open(device.__file__).read().split("\n")
        for line, fn in uncovered_lines().items():
            print("%5d  %-18s %s" % (line, fn, src[line - 1]))
        return 0
    got = text(sweep())
    if args.check:
        same = got == open(GOLDEN).read()
        print("identical" if same else "DIFFERENT from %s" % GOLDEN)
        return 0 if same else 1
    with open(GOLDEN, "w") as f:
        f.write(got)
    print("%d cases, %d bytes -> %s" % (got.count("\n") - 2, len(got), GOLDEN))
    return 0


if __name__ == "__main__":
    sys.exit(main())
