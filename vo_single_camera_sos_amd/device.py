"""Thin, checked Python face of the C ABI: torch tensors are used only as device-memory
containers (data_ptr()) and for the stream handle.  Every method validates dtype, device,
contiguity and shape on the host before a kernel may touch the memory."""
import ctypes

import torch

from . import _lib
from ._lib import SosvoError, c_f32, c_p

NULL = c_p(0)


def _ptr(t):
    return c_p(t.data_ptr()) if t is not None else NULL


def _run_cols(cfg):
    """The columns of the table and the mask bits a batch configuration's front end takes: cfg.cols, or with
    SOSVO_FLAG_SEAM_FREE the padded panorama's (sosvo_unwrap_prepare_seam_free, sosvo_mask_bits_seam_free)."""
    return cfg.cols + (2 * _lib.SEAM_HALO if cfg.ransac_flags & _lib.FLAG_SEAM_FREE else 0)


def _check(t, dtype, name, shape=None, ndim=None):
    if not isinstance(t, torch.Tensor):
        raise SosvoError("%s: expected a torch tensor, got %r" % (name, type(t)))
    if not t.is_cuda:
        raise SosvoError("%s: must live on the GPU" % name)
    if t.dtype != dtype:
        raise SosvoError("%s: dtype %s, expected %s" % (name, t.dtype, dtype))
    if not t.is_contiguous():
        raise SosvoError("%s: must be contiguous" % name)
    if ndim is not None and t.dim() != ndim:
        raise SosvoError("%s: ndim %d, expected %d" % (name, t.dim(), ndim))
    if shape is not None:
        if len(shape) != t.dim() or any(s is not None and s != d for s, d in zip(shape, t.shape)):
            raise SosvoError("%s: shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
    return t


def _check_opt(t, dtype, name, shape=None, ndim=None):
    """An optional input: checked when given."""
    return t if t is None else _check(t, dtype, name, shape, ndim)


def _new(shape, dtype, dev, fill=None):
    """A fresh buffer: fill None = uninitialised, 0 = zeros, anything else = that value everywhere."""
    if fill is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if fill == 0:
        return torch.zeros(shape, dtype=dtype, device=dev)
    return torch.full(shape, fill, dtype=dtype, device=dev)


def _buf(t, dtype, name, shape, dev, fill=None):
    """An optional output: allocated when None, checked either way."""
    return _check(_new(shape, dtype, dev, fill) if t is None else t, dtype, name, shape)


def _struct_ptr(s):
    """A host struct (ctypes.Structure) as the void* the entry points take."""
    return ctypes.cast(ctypes.pointer(s), c_p)


class Record(object):
    """One buffer record of the C ABI, described once: (key, dtype, shape, fill) per field, in the order the entry points
    take the pointers.  A shape names the dimensions that the call decides ("F", "cap") and spells out the rest; they are
    bound by keyword at use (None: that dimension is not checked).  fill is what a buffer that device.py allocates holds
    before the call (_new).  Allocation, the checks -- also of the part of a record a reader takes, sub() -- and the
    pointer list all come from this one text."""

    def __init__(self, *fields):
        self.fields = fields
        self.keys = tuple(f[0] for f in fields)
        self._memo = (None, None)

    def sub(self, *keys):
        """The record of these fields only, in this record's order."""
        assert set(keys) <= set(self.keys)
        return Record(*[f for f in self.fields if f[0] in keys])

    def _bound(self, dims):
        """The fields with their shapes bound to `dims`.  The latest binding is kept: a hot loop asks for the same one call
        after call (one attribute, replaced whole: records are shared by the contexts of every host thread)."""
        memo = self._memo
        if memo[0] != dims:
            memo = self._memo = (dims, [(key, dtype, tuple([dims[d] if type(d) is str else d for d in shape]), fill)
                                        for key, dtype, shape, fill in self.fields])
        return memo[1]

    def alloc(self, dev, zeroed=False, **dims):
        """-> {key: fresh buffer}; zeroed: zeros everywhere instead of the fields' own fills."""
        return {key: _new(shape, dtype, dev, 0 if zeroed else fill) for key, dtype, shape, fill in self._bound(dims)}

    def check(self, rec, **dims):
        for key, dtype, shape, _ in self._bound(dims):
            _check(rec[key], dtype, key, shape)

    def fill(self, dev, given, **dims):
        """given: {key: tensor or None}, every None replaced by a fresh buffer, every field checked -> given."""
        for key, dtype, shape, fill in self._bound(dims):
            given[key] = _buf(given.get(key), dtype, key, shape, dev, fill)
        return given

    def of(self, dev, given, **dims):
        """The caller's record `given`, checked, or a fresh one where it is None."""
        if given is None:
            return self.fill(dev, {}, **dims)
        self.check(given, **dims)
        return given

    def ptrs(self, rec):
        """The pointers in ABI order (a field the record lacks: NULL)."""
        return [_ptr(rec.get(key)) for key in self.keys]


f32, f64, i32, u8, u32 = torch.float32, torch.float64, torch.int32, torch.uint8, torch.uint32

# what stereo_assemble writes per frame, and the parts f2f_assemble / f2f_assemble_tracked read
FRAME = Record(("m_top", f32, ("F", "cap", 2), 0), ("m_bot", f32, ("F", "cap", 2), 0), ("d_top", u8, ("F", "cap", 32), 0),
               ("d_bot", u8, ("F", "cap", 32), 0), ("X", f64, ("F", "cap", 3), 0), ("b_top", f64, ("F", "cap", 3), 0),
               ("b_bot", f64, ("F", "cap", 3), 0), ("M", i32, ("F",), 0), ("n_cand", i32, ("F",), 0))
FRAME_MATCHED = FRAME.sub("m_top", "m_bot", "X", "b_top", "b_bot", "M")
FRAME_TRACKED = FRAME.sub("m_top", "m_bot", "X", "M")
# what rgbd_assemble writes per frame
RGBD_FRAME = Record(("m", f32, ("F", "cap", 2), 0), ("d", u8, ("F", "cap", 32), 0), ("X", f64, ("F", "cap", 3), 0),
                    ("b", f64, ("F", "cap", 3), 0), ("M", i32, ("F",), 0))
RGBD_FRAME_READ = RGBD_FRAME.sub("m", "X", "b", "M")        # the part f2f_assemble_central reads (it checks none of it)
# the correspondences of f2f_assemble / f2f_assemble_tracked, and the central form of f2f_assemble_central
CORR = Record(("f", f64, ("NP", "cap", 3), 0), ("p", f64, ("NP", "cap", 3), 0), ("cam", i32, ("NP", "cap"), 0),
              ("q", i32, ("NP", "cap"), 0), ("t", i32, ("NP", "cap"), 0), ("n", i32, ("NP",), 0), ("n_top", i32, ("NP",), 0))
CORR_CENTRAL = CORR.sub("f", "p", "q", "t", "n")
# the result of ransac_abs_pose / ransac_rel_pose, with and without the per-hypothesis counts
RANSAC_COUNTED = Record(("T", f64, ("P", 3, 4), None), ("mask", u8, ("P", "S"), 0), ("idx", i32, ("P", "S"), -1),
                        ("n_inliers", i32, ("P",), None), ("info", i32, ("P", 4), None), ("counts", i32, ("P", "K"), None))
RANSAC = RANSAC_COUNTED.sub("T", "mask", "idx", "n_inliers", "info")
# the outputs of the per-mask detectors (detect_fast / detect_agast / detect_gft) and of the three ORB methods
DETECTED = Record(("kp", f32, ("P", "cap", 2), 0), ("n", i32, ("P",), 0), ("status", i32, ("P",), 0))
ORB = Record(("kp4", f32, ("P", "cap", 4), 0), ("resp", f32, ("P", "cap"), 0), ("n", i32, ("P",), 0),
             ("desc", u8, ("P", "cap", 32), 0), ("kp_xy", f32, ("P", "cap", 2), 0))
ORB_DETECTED, ORB_KP4, ORB_RESP_N = ORB.sub("kp4", "resp", "n"), ORB.sub("kp4"), ORB.sub("resp", "n")
ORB_KP4_N, ORB_DESC, ORB_DESCRIBED = ORB.sub("kp4", "n"), ORB.sub("desc"), ORB.sub("desc", "kp_xy")


def make_rig(pano_top, pano_bot, F_top, F_bot, min_range, max_range, stereo_min_disp=1.0, stereo_max_hdiff=2.5,
             f2f_max_hdiff=-1.0, pct_good_matches=1.0):
    """Host-side sosvo_rig.  pano_* = (cols, rows, pixel_size, cyl_height_max)."""
    r = _lib.Rig()
    for k in range(4):
        r.pano_top[k] = float(pano_top[k])
        r.pano_bot[k] = float(pano_bot[k])
    for k in range(3):
        r.F_top[k] = float(F_top[k])
        r.F_bot[k] = float(F_bot[k])
    r.min_range, r.max_range = float(min_range), float(max_range)
    r.stereo_min_disp, r.stereo_max_hdiff = float(stereo_min_disp), float(stereo_max_hdiff)
    r.f2f_max_hdiff, r.pct_good_matches = float(f2f_max_hdiff), float(pct_good_matches)
    return r


class GrayPyramid(object):
    """What Context.gray_pyramid returns and Context.track_lk reads: `gray` [NI,rows,cols] u8 (level 0, the caller's tensor),
    `upper` (the levels 1 .. levels - 1 back to back, flat u8), `levels`, the `row_range` the levels were built under, and
    `cyclic`: built by gray_pyramid_cyclic, the columns are one period."""

    def __init__(self, gray, upper, levels, row_range, cyclic=False):
        self.gray, self.upper, self.levels, self.row_range, self.cyclic = gray, upper, levels, row_range, bool(cyclic)

    def level(self, l):
        """Level l as a [NI, rows_l, cols_l] view."""
        NI, rows, cols = self.gray.shape
        if l == 0:
            return self.gray
        off = 0
        for k in range(1, l + 1):
            rows, cols = (rows + 1) // 2, (cols + 1) // 2
            if k < l:
                off += NI * rows * cols
        return self.upper[off:off + NI * rows * cols].view(NI, rows, cols)


class Context(object):
    """One sosvo_ctx bound to (device, stream).  Not shared between host threads."""

    def __init__(self, device=0, stream=None):
        self._lib = _lib.load()
        if not torch.cuda.is_available():
            raise SosvoError("no GPU visible: libsosvo needs an MI355X (gfx950); there is no CPU fallback")
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        self.stream = stream
        h = c_p()
        rc = self._lib.sosvo_create(ctypes.byref(h), int(device), c_p(stream.cuda_stream))
        if rc != 0:
            raise SosvoError("sosvo_create failed: %s" % _lib.STATUS_NAMES.get(rc, rc))
        self._h = h
        self.lk_options = _lib.LKOptions()   # what the context tracks with under SOSVO_FLAG_LK_F2F (set_lk_options)
        self.stereo_lk_options = _lib.StereoLKOptions()   # ... and refines with under SOSVO_FLAG_LK_STEREO

    def close(self):
        if getattr(self, "_h", None) is not None:
            self._lib.sosvo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, fn, *args):
        rc = fn(self._h, *args)
        if rc != 0:
            msg = self._lib.sosvo_last_error(self._h)
            raise SosvoError("%s -> %s: %s" % (fn.__name__, _lib.STATUS_NAMES.get(rc, rc),
                                               msg.decode() if msg else ""))

    # ---- plumbing ----------------------------------------------------------------------
    def set_hint_shared_device(self, on=True):
        """sosvo_set_hint(SOSVO_HINT_SHARED_DEVICE): other contexts' kernels run beside this one's (scheduling only)."""
        self._call(self._lib.sosvo_set_hint, _lib.HINT_SHARED_DEVICE, 1 if on else 0)

    def set_hint_match_unsplit(self, on=True):
        """sosvo_set_hint(SOSVO_HINT_MATCH_UNSPLIT): the matrix-core matchers walk the train range in one workgroup per query tile
        instead of splitting it (same keys, bit for bit; for A/B measurements)."""
        self._call(self._lib.sosvo_set_hint, _lib.HINT_MATCH_UNSPLIT, 1 if on else 0)

    def set_hint_rolling_narrow(self, on=True):
        """sosvo_set_hint(SOSVO_HINT_ROLLING_NARROW): the rolling image kernels in their one-column-per-lane form at every
        width (same bytes; for A/B measurements and the cross-check of the two forms)."""
        self._call(self._lib.sosvo_set_hint, _lib.HINT_ROLLING_NARROW, 1 if on else 0)

    def set_hint_score_fp64_only(self, on=True):
        """sosvo_set_hint(SOSVO_HINT_SCORE_FP64_ONLY): RANSAC scoring without its single-precision first tier (same counts;
        for A/B measurements and the cross-check of the two forms)."""
        self._call(self._lib.sosvo_set_hint, _lib.HINT_SCORE_FP64_ONLY, 1 if on else 0)

    def set_lk_options(self, lk=None):
        """sosvo_set_lk_options: the tracker's settings of the batch and sequence entry points under SOSVO_FLAG_LK_F2F (an
        LKOptions, a dict of its fields, or None = the defaults).  They change results; a refused value leaves the previous
        settings.  self.lk_options is what the context holds."""
        lk = _lib.LKOptions.of(lk)
        self._call(self._lib.sosvo_set_lk_options, ctypes.byref(_lib.LkOptionsStruct.of(lk)))
        self.lk_options = lk

    def set_stereo_lk_options(self, stereo_lk=None):
        """sosvo_set_stereo_lk_options: the settings of the static-stereo refinement of the batch and sequence entry points
        under SOSVO_FLAG_LK_STEREO (a StereoLKOptions, a dict of its fields, or None = the defaults).  They change results; a
        refused value leaves the previous settings.  self.stereo_lk_options is what the context holds."""
        o = _lib.StereoLKOptions.of(stereo_lk)
        self._call(self._lib.sosvo_set_stereo_lk_options, ctypes.byref(_lib.StereoLkOptionsStruct.of(o)))
        self.stereo_lk_options = o

    def set_stream(self, stream):
        """Enqueue on `stream` (a torch.cuda.Stream) from now on, e.g. the capture stream of a HIP graph."""
        self._call(self._lib.sosvo_set_stream, c_p(stream.cuda_stream))
        self.stream = stream

    def synchronize(self):
        self._call(self._lib.sosvo_synchronize)

    def timer_start(self):
        self._call(self._lib.sosvo_timer_start)

    def timer_stop(self):
        self._call(self._lib.sosvo_timer_stop)

    def timer_elapsed_ms(self):
        ms = c_f32()
        self._call(self._lib.sosvo_timer_elapsed_ms, ctypes.byref(ms))
        return float(ms.value)

    def debug_fill_scratch(self, byte=0xFF):
        """Test hook: overwrite the library's internal scratch memory of this context (results must not change)."""
        self._call(self._lib.sosvo_debug_fill_scratch, int(byte))

    def profile_enable(self, on=True):
        """Start (and clear) / stop the per-kernel HIP-event record."""
        self._call(self._lib.sosvo_profile_enable, 1 if on else 0)

    def profile_read(self):
        """-> list of (kernel label, milliseconds) for every launch since profile_enable(True)."""
        n = self._lib.sosvo_profile_count(self._h)
        buf = ctypes.create_string_buffer(128)
        ms = c_f32()
        out = []
        for i in range(n):
            self._call(self._lib.sosvo_profile_get, i, buf, 128, ctypes.byref(ms))
            out.append((buf.value.decode(), float(ms.value)))
        return out

    # ---- K1 / K2 / K3 ------------------------------------------------------------------
    def unwrap(self, omni, masks, map_x, map_y, pano=None):
        """omni [F,H,W,3] u8, masks [2,H,W] u8 or None, map_x/map_y [2,rows,cols] f32 ->
        pano [2,F,rows,cols,3] u8 (view-major)."""
        _check(omni, torch.uint8, "omni", (None, None, None, 3))
        F, H, W = omni.shape[0], omni.shape[1], omni.shape[2]
        _check_opt(masks, torch.uint8, "masks", (2, H, W))
        _check(map_x, torch.float32, "map_x", (2, None, None))
        rows, cols = map_x.shape[1], map_x.shape[2]
        _check(map_y, torch.float32, "map_y", (2, rows, cols))
        pano = _buf(pano, torch.uint8, "pano", (2, F, rows, cols, 3), omni.device)
        self._call(self._lib.sosvo_unwrap, _ptr(omni), _ptr(masks), _ptr(map_x), _ptr(map_y), F, H, W, rows, cols,
                   _ptr(pano))
        return pano

    def unwrap_prepare(self, masks, map_x, map_y, omni_shape):
        """Model constants -> packed unwrap table [2, rows, cols, 2] u32 (once per model).  omni_shape (H, W): at most
        16384 each and 3 * W * (H - 1) >= 8, the frame-size rule of the table form (include/sosvo.h)."""
        return self._unwrap_prepare(self._lib.sosvo_unwrap_prepare, 0, masks, map_x, map_y, omni_shape)

    def _unwrap_prepare(self, entry, halo, masks, map_x, map_y, omni_shape):
        H, W = omni_shape
        _check_opt(masks, torch.uint8, "masks", (2, H, W))
        _check(map_x, torch.float32, "map_x", (2, None, None))
        rows, cols = map_x.shape[1], map_x.shape[2]
        _check(map_y, torch.float32, "map_y", (2, rows, cols))
        table = torch.empty((2, rows, cols + 2 * halo, 2), dtype=torch.uint32, device=map_x.device)
        self._call(entry, _ptr(masks), _ptr(map_x), _ptr(map_y), H, W, rows, cols, _ptr(table))
        return table

    # ---- the seam-free front end's stages -------------------------------------------------------
    def unwrap_prepare_seam_free(self, masks, map_x, map_y, omni_shape):
        """sosvo_unwrap_prepare_seam_free: the table [2, rows, cols + 80, 2] u32 of the maps padded by SEAM_HALO cyclic columns on
        either side -- byte for byte unwrap_prepare on such maps.  cols >= 40."""
        return self._unwrap_prepare(self._lib.sosvo_unwrap_prepare_seam_free, _lib.SEAM_HALO, masks, map_x, map_y, omni_shape)

    def mask_bits_seam_free(self, mask_bits, out=None):
        """sosvo_mask_bits_seam_free: mask_bits [nsets, rows, cols] u32 -> [nsets, rows, cols + 80], the masks in the columns
        [40, 40 + cols) and an empty halo: every original pixel is detected exactly once."""
        _check(mask_bits, torch.uint32, "mask_bits", (None, None, None))
        nsets, rows, cols = mask_bits.shape
        out = _buf(out, torch.uint32, "out", (nsets, rows, cols + 2 * _lib.SEAM_HALO), mask_bits.device)
        self._call(self._lib.sosvo_mask_bits_seam_free, _ptr(mask_bits), nsets, rows, cols, _ptr(out))
        return out

    def keypoints_unpad(self, kp, n, period):
        """sosvo_keypoints_unpad: the first n[p] keypoints of kp [nprob, cap, 2] f32 from a padded panorama's columns back to
        the period's, in place (float32: x - 40, + period if negative, - period if >= period, `period` itself is 0).  Rows at
        and beyond n[p], y and everything else are untouched."""
        _check(kp, torch.float32, "kp", (None, None, 2))
        nprob, cap = kp.shape[0], kp.shape[1]
        _check(n, torch.int32, "n", (nprob,))
        self._call(self._lib.sosvo_keypoints_unpad, _ptr(kp), _ptr(n), nprob, cap, int(period))
        return kp

    def gray_unpad(self, gray, cols, row_range=None, out=None):
        """sosvo_gray_unpad: gray [nimg, rows, cols + 80] u8 -> out [nimg, rows, cols], the interior columns.  row_range (int32
        [2,2] on the device, nimg even): only those rows of each view are written."""
        cols = int(cols)
        _check(gray, torch.uint8, "gray", (None, None, cols + 2 * _lib.SEAM_HALO))
        nimg, rows = gray.shape[0], gray.shape[1]
        out = _buf(out, torch.uint8, "out", (nimg, rows, cols), gray.device, 0)
        _check_opt(row_range, torch.int32, "row_range", (2, 2))
        self._call(self._lib.sosvo_gray_unpad, _ptr(gray), nimg, rows, cols, _ptr(row_range), _ptr(out))
        return out

    def unwrap_table(self, omni, table, pano=None):
        """omni [F,H,W,3] u8, table from unwrap_prepare -> pano [2,F,rows,cols,3] u8 (view-major)."""
        _check(omni, torch.uint8, "omni", (None, None, None, 3))
        F, H, W = omni.shape[0], omni.shape[1], omni.shape[2]
        _check(table, torch.uint32, "table", (2, None, None, 2))
        rows, cols = table.shape[1], table.shape[2]
        pano = _buf(pano, torch.uint8, "pano", (2, F, rows, cols, 3), omni.device)
        self._call(self._lib.sosvo_unwrap_table, _ptr(omni), _ptr(table), F, H, W, rows, cols, _ptr(pano))
        return pano

    def median_gray(self, img, ksize, gray=None):
        """img [..., rows, cols, 3] u8 -> gray [..., rows, cols] u8 (k x k median per channel, then BGR2GRAY)."""
        _check(img, torch.uint8, "img")
        if img.dim() < 3 or img.shape[-1] != 3:
            raise SosvoError("img: expected [..., rows, cols, 3]")
        rows, cols = img.shape[-3], img.shape[-2]
        nimg = int(img.numel() // (rows * cols * 3))
        gray = _buf(gray, torch.uint8, "gray", tuple(img.shape[:-1]), img.device)
        self._call(self._lib.sosvo_median_gray, _ptr(img), nimg, rows, cols, int(ksize), _ptr(gray))
        return gray

    def gray_rows_needed(self, mask_bits, nmask, edge, pattern, cos_a, sin_a):
        """Rows of the gray panoramas that GFT on the azimuthal masks + ORB.compute can reach: mask_bits
        [nsets,rows,cols] u32 -> row_range [nsets,2] i32 on the device (first row, last row + 1).  Model constant."""
        _check(mask_bits, torch.uint32, "mask_bits", (None, None, None))
        _check(pattern, torch.int8, "pattern")
        nsets, rows, cols = mask_bits.shape
        out = torch.zeros((nsets, 2), dtype=torch.int32, device=mask_bits.device)
        self._call(self._lib.sosvo_gray_rows_needed, _ptr(mask_bits), nsets, rows, cols, int(nmask), int(edge), _ptr(pattern),
                   float(cos_a), float(sin_a), _ptr(out))
        return out

    def unwrap_median_gray(self, omni, table, ksize, gray=None, row_range=None):
        """K1 + K2 + K3 fused: omni [F,H,W,3] u8, table from unwrap_prepare -> gray [2F,rows,cols] u8 (view-major);
        the colour panoramas are never materialised.  Same result as unwrap_table + median_gray.  row_range
        ([2,2] i32 from gray_rows_needed): only those rows of each view are computed and written."""
        _check(omni, torch.uint8, "omni", (None, None, None, 3))
        F, H, W = omni.shape[0], omni.shape[1], omni.shape[2]
        _check(table, torch.uint32, "table", (2, None, None, 2))
        rows, cols = table.shape[1], table.shape[2]
        gray = _buf(gray, torch.uint8, "gray", (2 * F, rows, cols), omni.device)
        if row_range is None:
            self._call(self._lib.sosvo_unwrap_median_gray, _ptr(omni), _ptr(table), F, H, W, rows, cols, int(ksize), _ptr(gray))
        else:
            _check(row_range, torch.int32, "row_range", (2, 2))
            self._call(self._lib.sosvo_unwrap_median_gray_rows, _ptr(omni), _ptr(table), F, H, W, rows, cols, int(ksize),
                       _ptr(row_range), _ptr(gray))
        return gray

    def detect_agast(self, gray, mask_bits, images_per_maskset, nmask, cap, threshold=10, kp=None, n=None, status=None):
        """AGAST (OAST 9/16) + its block-maximum NMS per azimuthal mask, raster order; arguments as detect_fast."""
        return self.detect_fast(gray, mask_bits, images_per_maskset, nmask, cap, threshold, kp, n, status, _agast=True)

    @staticmethod
    def _masked_images(gray, mask_bits, images_per_maskset):
        """What the per-mask detectors check of their inputs: gray [NI,rows,cols] u8 and mask_bits with enough sets for the
        images -> (NI, rows, cols)."""
        _check(gray, torch.uint8, "gray", ndim=3)
        NI, rows, cols = gray.shape
        _check(mask_bits, torch.uint32, "mask_bits", (None, rows, cols))
        if mask_bits.shape[0] * images_per_maskset < NI:
            raise SosvoError("mask_bits has too few sets for %d images" % NI)
        return NI, rows, cols

    def detect_fast(self, gray, mask_bits, images_per_maskset, nmask, cap, threshold=10, kp=None, n=None, status=None,
                    _agast=False):
        """FAST-9/16 + NMS per azimuthal mask, raster order: gray [NI,rows,cols] u8, mask_bits [nsets,rows,cols] u32
        -> kp [NI*nmask, cap, 2] f32, n [NI*nmask] i32, status [NI*nmask] i32."""
        NI, rows, cols = self._masked_images(gray, mask_bits, images_per_maskset)
        kp, n, status = DETECTED.fill(gray.device, dict(kp=kp, n=n, status=status), P=NI * nmask, cap=cap).values()
        self._call(self._lib.sosvo_detect_agast if _agast else self._lib.sosvo_detect_fast, _ptr(gray), _ptr(mask_bits), NI,
                   int(images_per_maskset), rows, cols, int(nmask), int(threshold), int(cap), _ptr(kp), _ptr(n), _ptr(status))
        return kp, n, status

    # ---- K4 / K6 -----------------------------------------------------------------------
    def detect_gft(self, gray, mask_bits, images_per_maskset, nmask, cap, quality=0.01, min_distance=5.0,
                   max_corners=1000, kp=None, n=None, status=None):
        """gray [NI,rows,cols] u8, mask_bits [nsets,rows,cols] u32 (as int32 bit patterns are not accepted: use
        torch.uint32) -> kp [NI*nmask, cap, 2] f32, n [NI*nmask] i32, status [NI*nmask] i32."""
        NI, rows, cols = self._masked_images(gray, mask_bits, images_per_maskset)
        kp, n, status = DETECTED.fill(gray.device, dict(kp=kp, n=n, status=status), P=NI * nmask, cap=cap).values()
        self._call(self._lib.sosvo_detect_gft, _ptr(gray), _ptr(mask_bits), NI, int(images_per_maskset), rows, cols,
                   int(nmask), float(quality), float(min_distance), int(max_corners), int(cap), _ptr(kp), _ptr(n),
                   _ptr(status))
        return kp, n, status

    def describe_orb(self, gray, kp, n, nmask, pattern, cos_a, sin_a, edge=31, desc=None, row_range=None):
        """Compacts kp/n in place (border rule) and returns desc [NI*nmask, cap, 32] u8.  row_range (int32 [2,2] on the
        device, from gray_rows_needed): blur only the rows a descriptor can read."""
        _check(gray, torch.uint8, "gray", ndim=3)
        NI, rows, cols = gray.shape
        P = NI * nmask
        _check(kp, torch.float32, "kp", (P, None, 2))
        cap = kp.shape[1]
        _check(n, torch.int32, "n", (P,))
        _check(pattern, torch.int8, "pattern", (512, 2))
        desc = ORB_DESC.fill(gray.device, dict(desc=desc), P=P, cap=cap)["desc"]
        _check_opt(row_range, torch.int32, "row_range", (2, 2))
        self._call(self._lib.sosvo_describe_orb_rows, _ptr(gray), NI, rows, cols, int(nmask), cap, _ptr(kp), _ptr(n),
                   float(cos_a), float(sin_a), _ptr(pattern), int(edge), _ptr(row_range), _ptr(desc))
        return desc

    def detect_gft_candidates(self, gray, mask_bits, images_per_maskset, nmask):
        """sosvo_detect_gft_candidates: the corner-response half of detect_gft.  gray [NI,rows,cols] u8, mask_bits
        [NI/images_per_maskset, rows, cols] u32 -> dict(strip_w, strips, nchunks, chunk_rows, wcap, regions, cand
        [regions, wcap, 2] u32 (response bits, y << 16 | x), wcnt [regions] u32, mstat [NI*nmask, 5] u32)."""
        NI, rows, cols = self._masked_images(gray, mask_bits, images_per_maskset)
        geo = (ctypes.c_int32 * 6)()
        args = (_ptr(gray), _ptr(mask_bits), NI, int(images_per_maskset), rows, cols, int(nmask), geo)
        self._call(self._lib.sosvo_detect_gft_candidates, *(args + (NULL, NULL, NULL)))
        strip_w, strips, nchunks, chunk_rows, wcap, regions = [int(v) for v in geo]
        cand = torch.zeros((regions, wcap, 2), dtype=torch.uint32, device=gray.device)
        wcnt = torch.zeros((regions,), dtype=torch.uint32, device=gray.device)
        mstat = torch.zeros((NI * int(nmask), 5), dtype=torch.uint32, device=gray.device)
        self._call(self._lib.sosvo_detect_gft_candidates, *(args + (_ptr(cand), _ptr(wcnt), _ptr(mstat))))
        return dict(strip_w=strip_w, strips=strips, nchunks=nchunks, chunk_rows=chunk_rows, wcap=wcap, regions=regions,
                    cand=cand, wcnt=wcnt, mstat=mstat)

    def gauss7(self, gray, nimg, rows, cols, out=None, img_stride=None, out_stride=None, row_range=None):
        """sosvo_gauss7: the descriptor stage's 7x7 sigma-2 blur on its own.  gray and out are FLAT u8 tensors that hold image
        i at element i * img_stride / i * out_stride (default rows * cols: a dense [nimg, rows, cols] batch, which may also
        be passed as such); only the images' own bytes are read and written.  row_range (int32 [2,2] on the device, nimg
        even): only those rows of each view are written.  Returns out."""
        nimg, rows, cols = int(nimg), int(rows), int(cols)
        px = rows * cols
        img_stride = px if img_stride is None else int(img_stride)
        out_stride = px if out_stride is None else int(out_stride)
        _check(gray, torch.uint8, "gray")
        if out is None:
            out = torch.zeros(max(nimg - 1, 0) * out_stride + px, dtype=torch.uint8, device=gray.device)
        _check(out, torch.uint8, "out")
        if nimg < 0 or rows < 1 or cols < 1 or img_stride < px or out_stride < px:
            raise SosvoError("gauss7: nimg >= 0, rows, cols >= 1 and strides >= rows * cols")
        if nimg > 0 and (gray.numel() < (nimg - 1) * img_stride + px or out.numel() < (nimg - 1) * out_stride + px):
            raise SosvoError("gauss7: a buffer is shorter than (nimg - 1) * stride + rows * cols")
        _check_opt(row_range, torch.int32, "row_range", (2, 2))
        self._call(self._lib.sosvo_gauss7, _ptr(gray), nimg, rows, cols, img_stride, _ptr(out), out_stride, _ptr(row_range))
        return out

    def refine_subpix(self, gray, kp, n, nmask, half=5, max_iter=_lib.SUBPIX_MAX_ITER, eps=_lib.SUBPIX_EPS, row_range=None):
        """cv2.cornerSubPix in exact integers (sosvo_refine_subpix): refines kp [NI*nmask, cap, 2] f32 in place on gray
        [NI,rows,cols] u8, the image the detector saw; n and the rows beyond it are untouched.  half 2 .. 5; row_range
        (int32 [2,2] on the device, from gray_rows_needed): samples are clamped to those rows of each view."""
        _check(gray, torch.uint8, "gray", ndim=3)
        NI, rows, cols = gray.shape
        P = NI * nmask
        _check(kp, torch.float32, "kp", (P, None, 2))
        _check(n, torch.int32, "n", (P,))
        _check_opt(row_range, torch.int32, "row_range", (2, 2))
        self._call(self._lib.sosvo_refine_subpix, _ptr(gray), NI, rows, cols, int(nmask), kp.shape[1], _ptr(kp), _ptr(n),
                   int(half), int(max_iter), float(eps), _ptr(row_range))
        return kp

    # ---- pyramidal Lucas-Kanade tracking --------------------------------------------------
    def gray_pyramid(self, gray, levels, row_range=None, out=None):
        """sosvo_gray_pyramid: the levels 1 .. levels - 1 of gray [NI,rows,cols] u8 (level 0 is `gray` itself, not copied) ->
        a GrayPyramid, what track_lk reads.  row_range (int32 [2,2] on the device, view-major) as for refine_subpix: only the
        rows a level inherits from it are computed.  out: a GrayPyramid of the same sizes to refill (no allocation)."""
        return self._gray_pyramid(False, gray, levels, row_range, out)

    def gray_pyramid_cyclic(self, gray, levels, row_range=None, out=None):
        """sosvo_gray_pyramid_cyclic: gray_pyramid for the panoramas of a full circle -- column `cols` is column 0 again, the
        column index wraps where gray_pyramid's clamps; cols must be a multiple of 2^(levels - 1).  -> a GrayPyramid with
        cyclic = True, which track_lk then tracks around the circle."""
        return self._gray_pyramid(True, gray, levels, row_range, out)

    def _gray_pyramid(self, cyclic, gray, levels, row_range, out):
        _check(gray, torch.uint8, "gray", ndim=3)
        NI, rows, cols = gray.shape
        nbytes = _lib.gray_pyramid_bytes(NI, rows, cols, levels)     # (SosvoError for sizes / levels out of range)
        _check_opt(row_range, torch.int32, "row_range", (2, 2))
        upper = out.upper if out is not None else torch.zeros((nbytes,), dtype=torch.uint8, device=gray.device)
        _check(upper, torch.uint8, "out.upper", (nbytes,))
        self._call(self._lib.sosvo_gray_pyramid_cyclic if cyclic else self._lib.sosvo_gray_pyramid, _ptr(gray), NI, rows, cols,
                   int(levels), _ptr(row_range), _ptr(upper) if nbytes else NULL)
        return GrayPyramid(gray, upper, int(levels), row_range, cyclic)

    def track_lk(self, pyr, prev_img, next_img, prev_pts, n, half=10, max_iter=30, eps=0.01, min_eig=1e-4, next_pts=None,
                 fb_max=None, out=None, cyclic=None):
        """sosvo_track_lk: problem p tracks prev_pts[p, :n[p]] ([NP,cap,2] f32) from image prev_img[p] to image next_img[p]
        ([NP] i32 on the device) of the GrayPyramid `pyr` -> (next_pts [NP,cap,2] f32, status [NP,cap] u8, err [NP,cap] f32).
        next_pts: given = the starting guesses (SOSVO_LK_INITIAL_FLOW), overwritten with the results.  fb_max: None, or the
        forward-backward check's bound in pixels; then the 4-tuple (next_pts, status, err, back).  out: buffers to reuse, in
        the order of the result (out[0] is not read when next_pts is given); rows at and beyond n[p] of every output are
        untouched.  cyclic: SOSVO_LK_CYCLIC_COLUMNS -- x is a position on the circle, results in [0, cols); None: as `pyr`
        was built (gray_pyramid_cyclic: True)."""
        if not isinstance(pyr, GrayPyramid):
            raise SosvoError("pyr: expected the result of gray_pyramid")
        NI, rows, cols = pyr.gray.shape
        _check(prev_pts, torch.float32, "prev_pts", (None, None, 2))
        NP, cap = prev_pts.shape[:2]
        _check(prev_img, torch.int32, "prev_img", (NP,))
        _check(next_img, torch.int32, "next_img", (NP,))
        _check(n, torch.int32, "n", (NP,))
        flags = _lib.LK_CYCLIC_COLUMNS if (pyr.cyclic if cyclic is None else cyclic) else 0
        if next_pts is not None:
            flags |= _lib.LK_INITIAL_FLOW
        else:
            next_pts = out[0] if out is not None else torch.zeros_like(prev_pts)
        _check(next_pts, torch.float32, "next_pts", (NP, cap, 2))
        dev = prev_pts.device
        status = _buf(out[1] if out is not None else None, torch.uint8, "status", (NP, cap), dev, 0)
        err = _buf(out[2] if out is not None else None, torch.float32, "err", (NP, cap), dev, 0)
        back = None
        if fb_max is not None:
            back = out[3] if out is not None and len(out) > 3 else torch.zeros_like(prev_pts)
            _check(back, torch.float32, "back", (NP, cap, 2))
        self._call(self._lib.sosvo_track_lk, _ptr(pyr.gray), _ptr(pyr.upper) if pyr.upper.numel() else NULL, NI, rows, cols,
                   pyr.levels, _ptr(pyr.row_range), _ptr(prev_img), _ptr(next_img), NP, cap, _ptr(prev_pts), _ptr(n), int(half),
                   int(max_iter), float(eps), float(min_eig), flags, _ptr(next_pts), _ptr(status), _ptr(err), _ptr(back),
                   0.0 if fb_max is None else float(fb_max))
        return (next_pts, status, err) if fb_max is None else (next_pts, status, err, back)

    def refine_stereo_lk(self, gray, kp_top, n_top, kp_bot, n_bot, keys, nmask, stereo_min_disp=-1.0, stereo_max_hdiff=0.0,
                         stereo_lk=None, row_range=None, status=None):
        """sosvo_refine_stereo_lk: the bottom keypoint of every matched top / bottom pair is tracked from the top view's image
        into the bottom view's (one level, the matcher's partner as the initial flow) and moved IN PLACE where the result is
        accepted.  gray [2F,rows,cols] u8 view-major; kp_top, kp_bot [F*nmask, cap, 2] f32; n_top, n_bot [F*nmask] i32; keys
        [F*nmask, cap(, 1)] u32 in query order (query = bottom); stereo_min_disp / stereo_max_hdiff: the rig's gates for the
        pre-gate (the defaults disable it); stereo_lk: a StereoLKOptions / dict / None = the defaults; row_range as for
        refine_subpix -> (kp_bot, status [F*nmask, cap] u8)."""
        o = _lib.StereoLKOptions.of(stereo_lk)
        _check(gray, torch.uint8, "gray", ndim=3)
        NI, rows, cols = gray.shape
        if NI % 2:
            raise SosvoError("gray: expected the top and bottom views' images, view-major (an even count)")
        P = (NI // 2) * int(nmask)
        _check(kp_bot, torch.float32, "kp_bot", (P, None, 2))
        cap = kp_bot.shape[1]
        _check(kp_top, torch.float32, "kp_top", (P, cap, 2))
        _check(n_top, torch.int32, "n_top", (P,))
        _check(n_bot, torch.int32, "n_bot", (P,))
        _check(keys, torch.uint32, "keys")
        if tuple(keys.shape) not in ((P, cap), (P, cap, 1)):
            raise SosvoError("keys: expected shape %r (k = 1), got %r" % ((P, cap), tuple(keys.shape)))
        _check_opt(row_range, torch.int32, "row_range", (2, 2))
        status = _buf(status, torch.uint8, "status", (P, cap), gray.device, 0)
        opt = _lib.StereoLkOptionsStruct.of(o)
        self._call(self._lib.sosvo_refine_stereo_lk, _ptr(gray), NI, rows, cols, _ptr(row_range), int(nmask), cap, _ptr(kp_top),
                   _ptr(n_top), _ptr(kp_bot), _ptr(n_bot), _ptr(keys), float(stereo_min_disp), float(stereo_max_hdiff),
                   _struct_ptr(opt), _ptr(status))
        return kp_bot, status

    def f2f_assemble_tracked(self, rig, frames, ref_frame, trk_top, trk_bot, st_top, st_bot, corr_cap, out=None, cyclic=False):
        """sosvo_f2f_assemble_tracked: frames = dict from stereo_assemble (m_top, m_bot, X, M); ref_frame [NP] i32; trk_*
        [NP, frame_cap, 2] f32 and st_* [NP, frame_cap] u8 from track_lk -> the dict of f2f_assemble (q = -1).  cyclic:
        sosvo_f2f_assemble_tracked_cyclic, the |du| gate around the circle (period = the rig's pano_top[0] / pano_bot[0])."""
        F, frame_cap = frames["m_top"].shape[0], frames["m_top"].shape[1]
        NP = ref_frame.shape[0]
        _check(ref_frame, torch.int32, "ref_frame", (NP,))
        FRAME_TRACKED.check(frames, F=F, cap=frame_cap)
        for name, t in (("trk_top", trk_top), ("trk_bot", trk_bot)):
            _check(t, torch.float32, name, (NP, frame_cap, 2))
        for name, t in (("st_top", st_top), ("st_bot", st_bot)):
            _check(t, torch.uint8, name, (NP, frame_cap))
        out = CORR.of(ref_frame.device, out, NP=NP, cap=corr_cap)
        self._call(self._lib.sosvo_f2f_assemble_tracked_cyclic if cyclic else self._lib.sosvo_f2f_assemble_tracked,
                   _struct_ptr(rig), *FRAME_TRACKED.ptrs(frames), frame_cap, _ptr(ref_frame), _ptr(trk_top), _ptr(trk_bot),
                   _ptr(st_top), _ptr(st_bot), NP, corr_cap, *CORR.ptrs(out))
        return out

    # ---- K5 / K6' ----------------------------------------------------------------------
    def orb_pyramid_pixels(self, rows, cols):
        return int(self._lib.sosvo_orb_pyramid_pixels(int(rows), int(cols)))

    def orb_mask_pyramid(self, mask_bits, nmask):
        """mask_bits [nsets, rows, cols] u32 -> mask_pyr [nsets, pyramid_pixels] u32 (once per model)."""
        _check(mask_bits, torch.uint32, "mask_bits", ndim=3)
        nsets, rows, cols = mask_bits.shape
        out = torch.zeros((nsets, self.orb_pyramid_pixels(rows, cols)), dtype=torch.uint32, device=mask_bits.device)
        self._call(self._lib.sosvo_orb_mask_pyramid, _ptr(mask_bits), nsets, rows, cols, int(nmask), _ptr(out))
        return out

    def detect_orb(self, gray, mask_pyr, images_per_maskset, nmask, nfeatures, cap, kp4=None, resp=None, n=None):
        """gray [NI,rows,cols] u8 -> kp4 [NI*nmask, cap, 4] f32 (x, y, angle_deg, level), resp [NI*nmask, cap] f32,
        n [NI*nmask] i32."""
        _check(gray, torch.uint8, "gray", ndim=3)
        NI, rows, cols = gray.shape
        _check(mask_pyr, torch.uint32, "mask_pyr", (None, self.orb_pyramid_pixels(rows, cols)))
        if mask_pyr.shape[0] * images_per_maskset < NI:
            raise SosvoError("mask_pyr has too few sets for %d images" % NI)
        kp4, resp, n = ORB_DETECTED.fill(gray.device, dict(kp4=kp4, resp=resp, n=n), P=NI * nmask, cap=cap).values()
        self._call(self._lib.sosvo_detect_orb, _ptr(gray), _ptr(mask_pyr), NI, int(images_per_maskset), rows, cols,
                   int(nmask), int(nfeatures), int(cap), _ptr(kp4), _ptr(resp), _ptr(n))
        return kp4, resp, n

    def describe_orb_levels(self, gray, kp4, n, nmask, pattern, desc=None, kp_xy=None):
        """Compacts kp4 / n in place (31-px border rule); returns (desc [P,cap,32] u8, kp_xy [P,cap,2] f32)."""
        _check(gray, torch.uint8, "gray", ndim=3)
        NI, rows, cols = gray.shape
        P = NI * nmask
        ORB_KP4_N.check(dict(kp4=kp4, n=n), P=P, cap=None)
        cap = kp4.shape[1]
        _check(pattern, torch.int8, "pattern", (512, 2))
        desc, kp_xy = ORB_DESCRIBED.fill(gray.device, dict(desc=desc, kp_xy=kp_xy), P=P, cap=cap).values()
        self._call(self._lib.sosvo_describe_orb_levels, _ptr(gray), NI, rows, cols, int(nmask), cap, _ptr(kp4), _ptr(n),
                   _ptr(pattern), _ptr(desc), _ptr(kp_xy))
        return desc, kp_xy

    def detect_describe_orb(self, gray, mask_pyr, images_per_maskset, nmask, nfeatures, pattern, kp4, resp, n, desc,
                            kp_xy=None):
        """ORB detect + compute in one call on ONE shared pyramid (sosvo_detect_describe_orb): the outputs of detect_orb
        followed by describe_orb_levels (kp4 / n compacted by the border rule), all buffers caller-provided."""
        _check(gray, torch.uint8, "gray", ndim=3)
        NI, rows, cols = gray.shape
        P = NI * nmask
        _check(mask_pyr, torch.uint32, "mask_pyr", (None, self.orb_pyramid_pixels(rows, cols)))
        rec = dict(kp4=kp4, resp=resp, n=n, desc=desc, kp_xy=kp_xy)
        ORB_KP4.check(rec, P=P, cap=None)
        cap = kp4.shape[1]
        ORB_RESP_N.check(rec, P=P, cap=cap)
        _check(pattern, torch.int8, "pattern", (512, 2))
        (ORB_DESC if kp_xy is None else ORB_DESCRIBED).check(rec, P=P, cap=cap)
        self._call(self._lib.sosvo_detect_describe_orb, _ptr(gray), _ptr(mask_pyr), NI, int(images_per_maskset), rows, cols,
                   int(nmask), int(nfeatures), cap, _ptr(kp4), _ptr(resp), _ptr(n), _ptr(pattern), _ptr(desc),
                   _ptr(kp_xy) if kp_xy is not None else None)
        return kp4, resp, n, desc, kp_xy

    # ---- K7 ----------------------------------------------------------------------------
    def _hamming_args(self, q_desc, t_desc, nq, nt, q_slot, t_slot, keys, k=1, pos=None):
        """The checks the Hamming searches share: descriptor blocks, pos = (q_pos, t_pos) of a gated search, counts, the slot
        pair -> (P, Sq, St, keys [P, Sq, k] u32, allocated when None)."""
        _check(q_desc, torch.uint8, "q_desc", (None, None, _lib.DESC_BYTES))
        _check(t_desc, torch.uint8, "t_desc", (None, None, _lib.DESC_BYTES))
        Bq, Sq = q_desc.shape[0], q_desc.shape[1]
        Bt, St = t_desc.shape[0], t_desc.shape[1]
        if pos is not None:
            _check(pos[0], torch.float32, "q_pos", (Bq, Sq, 2))
            _check(pos[1], torch.float32, "t_pos", (Bt, St, 2))
        _check(nq, torch.int32, "nq", (Bq,))
        _check(nt, torch.int32, "nt", (Bt,))
        if (q_slot is None) != (t_slot is None):
            raise SosvoError("q_slot and t_slot go together")
        if q_slot is not None:
            P = q_slot.shape[0]
            _check(q_slot, torch.int32, "q_slot", (P,))
            _check(t_slot, torch.int32, "t_slot", (P,))
        else:
            if Bq != Bt:
                raise SosvoError("q_desc and t_desc must have the same number of blocks without slots")
            P = Bq
        return P, Sq, St, _buf(keys, torch.uint32, "keys", (P, Sq, k), q_desc.device)

    def match_hamming(self, q_desc, t_desc, nq, nt, k=1, keys=None, q_slot=None, t_slot=None):
        """q_desc [Bq, Sq, 32] u8, t_desc [Bt, St, 32] u8, nq [Bq] / nt [Bt] i32 -> keys [P, Sq, k] u32.
        Without slots P = Bq = Bt; with q_slot / t_slot [P] i32, problem p uses blocks q_slot[p] / t_slot[p]."""
        P, Sq, St, keys = self._hamming_args(q_desc, t_desc, nq, nt, q_slot, t_slot, keys, k)
        self._call(self._lib.sosvo_match_hamming, _ptr(q_desc), _ptr(t_desc), _ptr(nq), _ptr(nt), _ptr(q_slot),
                   _ptr(t_slot), P, Sq, St, int(k), _ptr(keys))
        return keys

    def match_hamming_gated(self, q_desc, t_desc, q_pos, t_pos, nq, nt, min_dv, max_du, max_distance=None, keys=None,
                            q_slot=None, t_slot=None, n_forward=None):
        """The 1-NN search of match_hamming among the trains that pass the pixel gate: q_pos [Bq, Sq, 2] / t_pos [Bt, St, 2]
        f32 are the (u, v) of the descriptor rows; gate = |u_t - u_q| <= max_du (if max_du > 0) and v_t - v_q >= min_dv (if
        min_dv >= 0), in double.  max_distance: None = no cap, else 0 .. 256.  Problems p >= n_forward (default: none) are
        reversed (v_q - v_t >= min_dv).  -> keys [P, Sq, 1] u32, KEY_NONE where no admissible train is within the cap."""
        P, Sq, St, keys = self._hamming_args(q_desc, t_desc, nq, nt, q_slot, t_slot, keys, 1, (q_pos, t_pos))
        self._call(self._lib.sosvo_match_hamming_gated, _ptr(q_desc), _ptr(t_desc), _ptr(q_pos), _ptr(t_pos), _ptr(nq), _ptr(nt),
                   _ptr(q_slot), _ptr(t_slot), P, P if n_forward is None else int(n_forward), Sq, St, float(min_dv),
                   float(max_du), 256 if max_distance is None else int(max_distance), _ptr(keys))
        return keys

    def match_hamming_gated_cyclic(self, q_desc, t_desc, q_pos, t_pos, nq, nt, max_du, period, max_distance=None, keys=None,
                                   q_slot=None, t_slot=None, n_forward=None):
        """match_hamming_gated in its frame-to-frame form (no v side) with the u side around the circle of `period` columns
        (sosvo_match_hamming_gated_cyclic): gate = d <= max_du or d >= period - max_du, d = |u_t - u_q| in double (if
        max_du > 0).  -> keys [P, Sq, 1] u32."""
        P, Sq, St, keys = self._hamming_args(q_desc, t_desc, nq, nt, q_slot, t_slot, keys, 1, (q_pos, t_pos))
        self._call(self._lib.sosvo_match_hamming_gated_cyclic, _ptr(q_desc), _ptr(t_desc), _ptr(q_pos), _ptr(t_pos), _ptr(nq),
                   _ptr(nt), _ptr(q_slot), _ptr(t_slot), P, P if n_forward is None else int(n_forward), Sq, St, float(max_du),
                   float(period), 256 if max_distance is None else int(max_distance), _ptr(keys))
        return keys

    def match_hamming_ratio(self, q_desc, t_desc, nq, nt, ratio_64ths, q_pos=None, t_pos=None, min_dv=-1.0, max_du=0.0,
                            max_distance=None, keys=None, rivals=None, q_slot=None, t_slot=None, n_forward=None):
        """The 1-NN search with Lowe's ratio rule fused in (sosvo_match_hamming_ratio): a forward problem's query keeps its
        key iff 64 * d1 < ratio_64ths * d2 against the runner-up (ratio_64ths 1 .. 63, 48 = 0.75).  q_pos / t_pos both None:
        the plain form (no runner-up: dropped); both given: the gated form of match_hamming_gated with min_dv / max_du /
        max_distance (no runner-up inside the gate: kept; the cap acts after the rule).  Problems p >= n_forward (default:
        none) are reversed and get no rule.  -> (keys [P, Sq, 1] u32, rivals [P, Sq, 1] u32): the filtered keys, KEY_NONE
        where dropped, and each query's runner-up key (unspecified in reversed rows)."""
        if (q_pos is None) != (t_pos is None):
            raise SosvoError("q_pos and t_pos go together")
        if q_pos is None and max_distance is not None:
            raise SosvoError("max_distance belongs to the gated form (q_pos / t_pos)")
        P, Sq, St, keys = self._hamming_args(q_desc, t_desc, nq, nt, q_slot, t_slot, keys, 1,
                                             None if q_pos is None else (q_pos, t_pos))
        rivals = _buf(rivals, torch.uint32, "rivals", (P, Sq, 1), q_desc.device)
        self._call(self._lib.sosvo_match_hamming_ratio, _ptr(q_desc), _ptr(t_desc), _ptr(q_pos), _ptr(t_pos), _ptr(nq), _ptr(nt),
                   _ptr(q_slot), _ptr(t_slot), P, P if n_forward is None else int(n_forward), Sq, St, float(min_dv),
                   float(max_du), 256 if max_distance is None else int(max_distance), int(ratio_64ths), _ptr(keys),
                   _ptr(rivals))
        return keys, rivals

    def match_1nn(self, q_desc, t_desc, nq, nt, *, ratio_64ths=0, rivals=None, gate=None, q_pos=None, t_pos=None, keys=None,
                  q_slot=None, t_slot=None, n_forward=None, period=None):
        """The Python twin of match_1nn in pipeline.hip: one best-match search, ONE library call.  ratio_64ths > 0: the ratio
        form (match_hamming_ratio), plain or, with a gate, gated; else with a gate: match_hamming_gated; else
        match_hamming(k=1), which has no reversed problems and so no n_forward.  gate: None or (min_dv, max_du, max_distance)
        on q_pos / t_pos.  period: None, or the period of a gate whose u side is cyclic (match_hamming_gated_cyclic: the
        frame-to-frame form, no v side, no ratio form; without a gate it is ignored, as the gate's values are).
        -> keys [P, Sq, 1] u32."""
        where = dict(keys=keys, q_slot=q_slot, t_slot=t_slot)
        if gate is not None and period is not None:
            if ratio_64ths or gate[0] >= 0:
                raise SosvoError("the cyclic gate has no ratio form and no v side")
            return self.match_hamming_gated_cyclic(q_desc, t_desc, q_pos, t_pos, nq, nt, gate[1], period, max_distance=gate[2],
                                                   n_forward=n_forward, **where)
        if ratio_64ths:
            g = dict(q_pos=q_pos, t_pos=t_pos, min_dv=gate[0], max_du=gate[1], max_distance=gate[2]) if gate is not None else {}
            return self.match_hamming_ratio(q_desc, t_desc, nq, nt, ratio_64ths, rivals=rivals, n_forward=n_forward, **g, **where)[0]
        if gate is not None:
            return self.match_hamming_gated(q_desc, t_desc, q_pos, t_pos, nq, nt, *gate, n_forward=n_forward, **where)
        return self.match_hamming(q_desc, t_desc, nq, nt, k=1, **where)

    def match_1nn_slots(self, desc, pos, n, q_slot, t_slot, keys, n_forward, *, ratio_64ths=0, rivals=None, gate=None, period=None):
        """The matching step, slot form: ONE search over the problems (q_slot[p], t_slot[p]) of one set of blocks (desc, pos, n).
        Problems p >= n_forward are the role-swapped twins of the forward ones (reversed gate, no ratio rule); when there are
        any, the forward keys are filtered to the mutual matches in place.  -> the forward keys, keys[:n_forward]."""
        self.match_1nn(desc, desc, n, n, ratio_64ths=ratio_64ths, rivals=rivals, gate=gate, q_pos=pos, t_pos=pos, keys=keys,
                       q_slot=q_slot, t_slot=t_slot, n_forward=n_forward, **({} if period is None else dict(period=period)))
        fwd = keys[:n_forward]
        if keys.shape[0] > n_forward:
            self.cross_check_matches(fwd, keys[n_forward:], n, n, q_slot=q_slot[:n_forward], t_slot=t_slot[:n_forward], keys_out=fwd)
        return fwd

    def match_1nn_two_launch(self, q_desc, t_desc, nq, nt, *, cross_check=False, keys_rev=None, ratio_64ths=0, rivals=None,
                             gate=None, q_pos=None, t_pos=None, keys=None, period=None):
        """The matching step, two-launch form: the forward search; with cross_check a second search with roles and positions
        swapped (every problem reversed: n_forward=0, never the ratio rule) into keys_rev, then the mutual filter on keys in
        place.  -> keys."""
        cyc = {} if period is None else dict(period=period)    # (the u side is symmetric: the swapped search takes it as well)
        keys = self.match_1nn(q_desc, t_desc, nq, nt, ratio_64ths=ratio_64ths, rivals=rivals, gate=gate, q_pos=q_pos, t_pos=t_pos,
                              keys=keys, **cyc)
        if cross_check:
            rev = self.match_1nn(t_desc, q_desc, nt, nq, gate=gate, q_pos=t_pos, t_pos=q_pos, keys=keys_rev, n_forward=0, **cyc)
            self.cross_check_matches(keys, rev, nq, nt, keys_out=keys)
        return keys

    def match_l2(self, q_desc, t_desc, nq, nt, k=1):
        """Float descriptors: q_desc [P, Sq, dim] f32, t_desc [P, St, dim] f32 -> keys [P, Sq, k] int64 holding the u64
        (float32 distance bits << 32 | train index); all ones (-1) if absent."""
        _check(q_desc, torch.float32, "q_desc", (None, None, None))
        P, Sq, dim = q_desc.shape
        _check(t_desc, torch.float32, "t_desc", (P, None, dim))
        St = t_desc.shape[1]
        _check(nq, torch.int32, "nq", (P,))
        _check(nt, torch.int32, "nt", (P,))
        keys = torch.empty((P, Sq, int(k)), dtype=torch.int64, device=q_desc.device)
        self._call(self._lib.sosvo_match_l2, _ptr(q_desc), _ptr(t_desc), _ptr(nq), _ptr(nt), P, Sq, St, int(dim), int(k),
                   _ptr(keys))
        return keys

    def match_radius(self, q_desc, t_desc, nq, nt, max_distance, cap, q_slot=None, t_slot=None):
        """radiusMatch: q_desc [Bq, Sq, 32] u8, t_desc [Bt, St, 32] u8 -> (keys [P, Sq, cap] u32 ascending,
        KEY_NONE padded; counts [P, Sq] i32 = matches within max_distance, may exceed cap)."""
        P, Sq, St, keys = self._hamming_args(q_desc, t_desc, nq, nt, q_slot, t_slot, None, int(cap))
        counts = torch.zeros((P, Sq), dtype=torch.int32, device=q_desc.device)
        self._call(self._lib.sosvo_match_radius, _ptr(q_desc), _ptr(t_desc), _ptr(nq), _ptr(nt), _ptr(q_slot), _ptr(t_slot),
                   P, Sq, St, int(max_distance), int(cap), _ptr(keys), _ptr(counts))
        return keys, counts

    def cross_check_matches(self, keys_fwd, keys_rev, nq, nt, q_slot=None, t_slot=None, keys_out=None, n_kept=None):
        """cv2.BFMatcher(NORM_HAMMING, crossCheck=True) on 1-NN keys: keys_fwd [P, Sq, 1] u32 from match_hamming(k=1),
        keys_rev [P, St, 1] u32 from the same call with query and train (and the slots) swapped -> (keys_out [P, Sq, 1]
        with the keys of non-mutual matches replaced by KEY_NONE, n_kept [P] i32).  keys_out may be keys_fwd."""
        _check(keys_fwd, torch.uint32, "keys_fwd", (None, None, 1))
        P, Sq = keys_fwd.shape[0], keys_fwd.shape[1]
        _check(keys_rev, torch.uint32, "keys_rev", (P, None, 1))
        St = keys_rev.shape[1]
        _check(nq, torch.int32, "nq", ndim=1)
        _check(nt, torch.int32, "nt", ndim=1)
        if (q_slot is None) != (t_slot is None):
            raise SosvoError("q_slot and t_slot go together")
        if q_slot is not None:
            _check(q_slot, torch.int32, "q_slot", (P,))
            _check(t_slot, torch.int32, "t_slot", (P,))
        elif nq.shape[0] != P or nt.shape[0] != P:
            raise SosvoError("nq and nt must have one entry per problem without slots")
        keys_out = _buf(keys_out, torch.uint32, "keys_out", (P, Sq, 1), keys_fwd.device, _lib.KEY_NONE)
        n_kept = _buf(n_kept, torch.int32, "n_kept", (P,), keys_fwd.device)
        self._call(self._lib.sosvo_cross_check_matches, _ptr(keys_fwd), _ptr(keys_rev), _ptr(nq), _ptr(nt), _ptr(q_slot),
                   _ptr(t_slot), P, Sq, St, _ptr(keys_out), _ptr(n_kept))
        return keys_out, n_kept

    def sort_matches(self, keys, nq, order=None, q_slot=None):
        """keys [P, Sq, 1] u32 (1-NN), nq i32 (per block) -> order [P, Sq] i32 (query index by rank)."""
        _check(keys, torch.uint32, "keys", (None, None, 1))
        P, Sq = keys.shape[0], keys.shape[1]
        _check(nq, torch.int32, "nq", ndim=1)
        if q_slot is not None:
            _check(q_slot, torch.int32, "q_slot", (P,))
        elif nq.shape[0] != P:
            raise SosvoError("nq must have one entry per problem without q_slot")
        order = _buf(order, torch.int32, "order", (P, Sq), keys.device, -1)
        self._call(self._lib.sosvo_sort_matches, _ptr(keys), _ptr(nq), _ptr(q_slot), P, Sq, _ptr(order))
        return order

    # ---- K8 / K10 / K9 -----------------------------------------------------------------
    def _rig_cams(self, cam, cam_off, cam_rot, P, S):
        """Validate the optional non-central rig description; returns (cam_ptr, off_ptr, rot_ptr, ncam)."""
        if cam is None:
            return NULL, NULL, NULL, 1
        _check(cam, torch.int32, "cam", (P, S))
        _check(cam_off, torch.float64, "cam_off", (None, 3))
        ncam = cam_off.shape[0]
        _check(cam_rot, torch.float64, "cam_rot", (ncam, 3, 3))
        if not 1 <= ncam <= 8:
            raise SosvoError("ncam %d out of range 1..8" % ncam)
        return _ptr(cam), _ptr(cam_off), _ptr(cam_rot), ncam

    def ransac_abs_pose(self, f, p, n, thr, max_iter, seed=0, adaptive=False, cam=None, cam_off=None,
                        cam_rot=None, cam_rot_identity=False, want_counts=False, out=None, epnp=False, gp3p=False, twopt=False,
                        seeds=None):
        """f, p [P, S, 3] f64, n [P] i32 (+ cam [P, S] i32, cam_off [C,3], cam_rot [C,3,3]) ->
        dict(T [P,3,4], mask [P,S] u8, idx [P,S] i32, n_inliers [P] i32, info [P,4] i32[, counts [P,max_iter]]).
        `out` may carry preallocated result tensors (same keys) to avoid allocations in a hot loop.
        seeds: one seed per problem (sosvo_ransac_abs_pose_seeds; see ransac_abs_pose_seeds) instead of seed + b."""
        _check(f, torch.float64, "f", (None, None, 3))
        P, S = f.shape[0], f.shape[1]
        _check(p, torch.float64, "p", (P, S, 3))
        _check(n, torch.int32, "n", (P,))
        cam_p, off_p, rot_p, ncam = self._rig_cams(cam, cam_off, cam_rot, P, S)
        dev = f.device
        if out is None:
            out = (RANSAC_COUNTED if want_counts else RANSAC).alloc(dev, P=P, S=S, K=int(max_iter))
        (RANSAC if out.get("counts") is None else RANSAC_COUNTED).check(out, P=P, S=S, K=int(max_iter))
        flags = (_lib.FLAG_CAM_ROT_IDENTITY if cam_rot_identity else 0) | (_lib.FLAG_EPNP if epnp else 0) | \
            (_lib.FLAG_GP3P if gp3p else 0) | (_lib.FLAG_TWOPT if twopt else 0)
        if seeds is not None:
            if not isinstance(seeds, torch.Tensor):   # host integers (any 64-bit pattern) -> device, as int64 bits
                import numpy as np
                seeds = torch.from_numpy(np.array([int(v) & (2 ** 64 - 1) for v in seeds], dtype=np.uint64).view(np.int64)).to(dev)
            if seeds.dtype not in (torch.int64, getattr(torch, "uint64", torch.int64)) or tuple(seeds.shape) != (P,) \
                    or not seeds.is_contiguous() or seeds.device != dev:
                raise SosvoError("seeds: [P] 64-bit integers, contiguous, on the problems' device")
            self._call(self._lib.sosvo_ransac_abs_pose_seeds, _ptr(f), _ptr(p), cam_p, off_p, rot_p, ncam, flags,
                       _ptr(n), P, S, float(thr), int(max_iter), 1 if adaptive else 0, _ptr(seeds), *RANSAC_COUNTED.ptrs(out))
            return out
        self._call(self._lib.sosvo_ransac_abs_pose, _ptr(f), _ptr(p), cam_p, off_p, rot_p, ncam, flags,
                   _ptr(n), P, S, float(thr), int(max_iter), 1 if adaptive else 0, int(seed) & (2 ** 64 - 1),
                   *RANSAC_COUNTED.ptrs(out))
        return out

    def ransac_abs_pose_seeds(self, f, p, n, thr, max_iter, seeds, **kwargs):
        """ransac_abs_pose with problem b sampling with seeds[b] ([P] device tensor of 64-bit integers, or host integers)
        instead of seed + b: the problems of one call may belong to different sequences."""
        if seeds is None:
            raise SosvoError("seeds: one per problem")
        return self.ransac_abs_pose(f, p, n, thr, max_iter, seeds=seeds, **kwargs)

    def ransac_rel_pose(self, f1, f2, n, thr, max_iter, algorithm=_lib.REL_EIGHTPT, seed=0, adaptive=False, want_counts=False):
        """f1, f2 [P, S, 3] f64 (bearings of the same features from viewpoints 1 and 2), n [P] i32 ->
        dict(T [P,3,4] (pose of viewpoint 2 in frame 1, |t| = 1), mask, idx, n_inliers, info[, counts])."""
        _check(f1, torch.float64, "f1", (None, None, 3))
        P, S = f1.shape[0], f1.shape[1]
        _check(f2, torch.float64, "f2", (P, S, 3))
        _check(n, torch.int32, "n", (P,))
        out = (RANSAC_COUNTED if want_counts else RANSAC).alloc(f1.device, P=P, S=S, K=int(max_iter))
        self._call(self._lib.sosvo_ransac_rel_pose, _ptr(f1), _ptr(f2), _ptr(n), P, S, int(algorithm), float(thr), int(max_iter),
                   1 if adaptive else 0, int(seed) & (2 ** 64 - 1), *RANSAC_COUNTED.ptrs(out))
        return out

    def refine_abs_pose(self, f, p, n, T, idx=None, m=None, cam=None, cam_off=None, cam_rot=None,
                        max_lm_iter=30, cost=None, iters=None):
        """In-place LM refinement of T [P,3,4]; returns (T, cost [P] f64, iters [P] i32)."""
        _check(f, torch.float64, "f", (None, None, 3))
        P, S = f.shape[0], f.shape[1]
        _check(p, torch.float64, "p", (P, S, 3))
        _check(n, torch.int32, "n", (P,))
        _check(T, torch.float64, "T", (P, 3, 4))
        cam_p, off_p, rot_p, ncam = self._rig_cams(cam, cam_off, cam_rot, P, S)
        if (idx is None) != (m is None):
            raise SosvoError("idx and m go together")
        if idx is not None:
            _check(idx, torch.int32, "idx", (P, S))
            _check(m, torch.int32, "m", (P,))
        cost = _buf(cost, torch.float64, "cost", (P,), f.device)
        iters = _buf(iters, torch.int32, "iters", (P,), f.device)
        self._call(self._lib.sosvo_refine_abs_pose, _ptr(f), _ptr(p), cam_p, off_p, rot_p, ncam, _ptr(n), P, S,
                   _ptr(idx), _ptr(m), int(max_lm_iter), _ptr(T), _ptr(cost), _ptr(iters))
        return T, cost, iters

    # ---- geometry ----------------------------------------------------------------------
    def pano_to_bearing(self, uv, cols, rows, pixel_size, cyl_height_max):
        """uv [n,2] f64 -> (az [n], el [n], bearing [n,3]) f64."""
        _check(uv, torch.float64, "uv", (None, 2))
        n = uv.shape[0]
        az = torch.empty((n,), dtype=torch.float64, device=uv.device)
        el = torch.empty((n,), dtype=torch.float64, device=uv.device)
        b = torch.empty((n, 3), dtype=torch.float64, device=uv.device)
        self._call(self._lib.sosvo_pano_to_bearing, _ptr(uv), n, float(cols), float(rows), float(pixel_size),
                   float(cyl_height_max), _ptr(az), _ptr(el), _ptr(b))
        return az, el, b

    def triangulate_midpoint(self, az_top, el_top, az_bot, el_bot, F_top, F_bot):
        n = az_top.shape[0]
        for name, t in (("az_top", az_top), ("el_top", el_top), ("az_bot", az_bot), ("el_bot", el_bot)):
            _check(t, torch.float64, name, (n,))
        X = torch.empty((n, 3), dtype=torch.float64, device=az_top.device)
        f1 = (ctypes.c_double * 3)(*[float(v) for v in F_top])
        f2 = (ctypes.c_double * 3)(*[float(v) for v in F_bot])
        self._call(self._lib.sosvo_triangulate_midpoint, _ptr(az_top), _ptr(el_top), _ptr(az_bot), _ptr(el_bot), n,
                   ctypes.cast(f1, c_p), ctypes.cast(f2, c_p), _ptr(X))
        return X

    def triangulate2(self, b1, b2, t12, R12):
        """b1, b2 [n,3] f64 unit bearings in frames 1 / 2, t12 (3), R12 (3x3) host -> X [n,3] in frame 1."""
        n = b1.shape[0]
        _check(b1, torch.float64, "b1", (n, 3))
        _check(b2, torch.float64, "b2", (n, 3))
        X = torch.empty((n, 3), dtype=torch.float64, device=b1.device)
        t = (ctypes.c_double * 3)(*[float(v) for v in t12])
        R = (ctypes.c_double * 9)(*[float(v) for row in R12 for v in row])
        self._call(self._lib.sosvo_triangulate2, _ptr(b1), _ptr(b2), n, ctypes.cast(t, c_p), ctypes.cast(R, c_p), _ptr(X))
        return X

    def range_filter(self, X, min_range, max_range):
        _check(X, torch.float64, "X", (None, 3))
        ok = torch.empty((X.shape[0],), dtype=torch.uint8, device=X.device)
        self._call(self._lib.sosvo_range_filter, _ptr(X), X.shape[0], float(min_range), float(max_range), _ptr(ok))
        return ok

    # ---- dense omnistereo ------------------------------------------
    def census(self, gray, cyclic=False):
        """sosvo_census_9x7: gray [NI,rows,cols] u8 -> the 62-bit census words [NI,rows,cols] (int64 holds the u64's bits)."""
        _check(gray, torch.uint8, "gray", ndim=3)
        out = torch.empty(gray.shape, dtype=torch.int64, device=gray.device)
        self._call(self._lib.sosvo_census_9x7, _ptr(gray), gray.shape[0], gray.shape[1], gray.shape[2],
                   _lib.DENSE_CYCLIC_COLUMNS if cyclic else 0, _ptr(out))
        return out

    def dense_stereo(self, top, bot, mask=None, *, options=None, want_volume=False, paths=4):
        """sosvo_dense_stereo: top, bot [n,rows,cols] u8 gray panoramas (the halves of unwrap_median_gray's output), mask
        [rows,cols] u8 or None, options a DenseOptions (None: the defaults) -> d16 [n,rows,cols] i16 (disparity in 1/16 row,
        -1 = invalid); with want_volume (d16, S [n,rows,cols,64] u16, the aggregated volume).  paths: 4, or 8 for the four
        diagonal paths as well (sosvo_dense_stereo_paths; needs P2 <= 8127); anything else raises
        ValueError before the call."""
        o = _lib.DenseOptions.of(options)
        paths = _lib.dense_paths(paths, o)
        _check(top, torch.uint8, "top", ndim=3)
        n, rows, cols = top.shape
        _check(bot, torch.uint8, "bot", (n, rows, cols))
        _check_opt(mask, torch.uint8, "mask", (rows, cols))
        d16 = torch.empty((n, rows, cols), dtype=torch.int16, device=top.device)
        S = torch.empty((n, rows, cols, _lib.DENSE_DISPARITIES), dtype=torch.uint16, device=top.device) if want_volume else None
        if paths == 4:
            self._call(self._lib.sosvo_dense_stereo, _ptr(top), _ptr(bot), n, rows, cols, _ptr(mask), o.min_disparity, o.P1, o.P2,
                       o.uniqueness, o.lr_max, o.flags, _ptr(d16), _ptr(S))
        else:
            self._call(self._lib.sosvo_dense_stereo_paths, _ptr(top), _ptr(bot), n, rows, cols, _ptr(mask), o.min_disparity, o.P1,
                       o.P2, o.uniqueness, o.lr_max, o.flags, paths, _ptr(d16), _ptr(S))
        return (d16, S) if want_volume else d16

    def dense_triangulate(self, rig, d16, min_disparity=1.0, max_disparity=0.0):
        """sosvo_dense_triangulate: d16 [n,rows,cols] i16 -> X [n,rows,cols,3] f64 in the rig's frame, NaN where the pixel has
        no disparity, min_disparity <= d16 / 16 <= max_disparity fails (the reference's two filters; max_disparity <= 0: no
        upper one), the bottom pixel leaves the panorama or the point fails the rig's range filter."""
        _check(d16, torch.int16, "d16", ndim=3)
        n, rows, cols = d16.shape
        lo = int(-(-float(min_disparity) * 16 // 1))                      # d16 >= ceil(16 min)
        hi = int(float(max_disparity) * 16 // 1) if max_disparity > 0 else 0   # d16 <= floor(16 max)
        if max_disparity > 0 and hi <= 0:      # (an upper gate below 1/16 row passes nothing; 0 would mean no gate)
            lo, hi = 1 << 20, 1
        X = torch.empty((n, rows, cols, 3), dtype=torch.float64, device=d16.device)
        self._call(self._lib.sosvo_dense_triangulate, _struct_ptr(rig), _ptr(d16), n, rows, cols, lo, hi, _ptr(X))
        return X

    def dense_speckle(self, d16, *, options, want_labels=False, out=None):
        """sosvo_dense_speckle: d16 [n,rows,cols] i16, options a SpeckleOptions (or a dict of its
        fields) -> the map with every component of at most max_size pixels set to -1, in `out` (None: a new tensor; d16
        itself: in place); with want_labels (map, labels [n,rows,cols] u32: the smallest row-major index of the pixel's
        component, 0xFFFFFFFF for an invalid pixel)."""
        o = _lib.SpeckleOptions.of(options)
        if o is None:
            raise ValueError("dense_speckle needs a SpeckleOptions: None means that the filter is off, and then there is no call")
        _check(d16, torch.int16, "d16", ndim=3)
        n, rows, cols = d16.shape
        if out is None:
            out = torch.empty_like(d16)
        _check(out, torch.int16, "out", (n, rows, cols))
        labels = torch.empty((n, rows, cols), dtype=torch.uint32, device=d16.device) if want_labels else None
        self._call(self._lib.sosvo_dense_speckle, _ptr(d16), n, rows, cols, o.max_size, o.max_diff, o.flags, _ptr(out), _ptr(labels))
        return (out, labels) if want_labels else out

    def rgbd_backproject(self, depth, u, v, fx, fy, cx, cy, focal_length_m, depth_is_Z):
        _check(depth, torch.float32, "depth", ndim=2)
        n = u.shape[0]
        _check(u, torch.int32, "u", (n,))
        _check(v, torch.int32, "v", (n,))
        xyz = torch.empty((n, 3), dtype=torch.float64, device=depth.device)
        b = torch.empty((n, 3), dtype=torch.float64, device=depth.device)
        self._call(self._lib.sosvo_rgbd_backproject, _ptr(depth), depth.shape[0], depth.shape[1], _ptr(u), _ptr(v), n,
                   float(fx), float(fy), float(cx), float(cy), float(focal_length_m), 1 if depth_is_Z else 0,
                   _ptr(xyz), _ptr(b))
        return xyz, b

    def stereo_assemble(self, rig, kp_top, kp_bot, desc_top, desc_bot, n_top, n_bot, keys, order, nframes, nmask,
                        out_cap, out=None):
        """Per-bucket stereo matches -> per-frame correspondences (see include/sosvo.h).
        kp_* [F*NM, cap, 2] f32, desc_* [F*NM, cap, 32] u8, n_* [F*NM] i32, keys [F*NM, cap, 1] u32,
        order [F*NM, cap] i32 -> dict(m_top, m_bot [F,out_cap,2] f32, d_top, d_bot [F,out_cap,32] u8,
        X, b_top, b_bot [F,out_cap,3] f64, M [F] i32, n_cand [F] i32)."""
        P = nframes * nmask
        _check(kp_top, torch.float32, "kp_top", (P, None, 2))
        cap = kp_top.shape[1]
        _check(kp_bot, torch.float32, "kp_bot", (P, cap, 2))
        _check(desc_top, torch.uint8, "desc_top", (P, cap, 32))
        _check(desc_bot, torch.uint8, "desc_bot", (P, cap, 32))
        _check(n_top, torch.int32, "n_top", (P,))
        _check(n_bot, torch.int32, "n_bot", (P,))
        _check(keys, torch.uint32, "keys", (P, cap, 1))
        _check(order, torch.int32, "order", (P, cap))
        F = nframes
        out = FRAME.of(kp_top.device, out, F=F, cap=out_cap)
        self._call(self._lib.sosvo_stereo_assemble, _struct_ptr(rig), _ptr(kp_top), _ptr(kp_bot),
                   _ptr(desc_top), _ptr(desc_bot), _ptr(n_top), _ptr(n_bot), _ptr(keys), _ptr(order), F, nmask, cap,
                   out_cap, *FRAME.ptrs(out))
        return out

    # ---- RGB-D variant ---------------------------------------------------------------------
    def rgbd_assemble(self, cam, kp, desc, n, depth, out_cap, out=None):
        """RGBDFrame.establish_keypoints after detection, batched.  cam: _lib.RgbdCam; kp [F,cap,2] f32,
        desc [F,cap,32] u8, n [F] i32, depth [F,rows,cols] f32 -> dict(m [F,out_cap,2] f32, d [F,out_cap,32] u8,
        X, b [F,out_cap,3] f64, M [F] i32)."""
        _check(kp, torch.float32, "kp", (None, None, 2))
        F, cap = kp.shape[0], kp.shape[1]
        _check(desc, torch.uint8, "desc", (F, cap, 32))
        _check(n, torch.int32, "n", (F,))
        _check(depth, torch.float32, "depth", (F, None, None))
        rows, cols = depth.shape[1], depth.shape[2]
        out = RGBD_FRAME.of(kp.device, out, F=F, cap=out_cap)
        self._call(self._lib.sosvo_rgbd_assemble, _struct_ptr(cam), _ptr(kp), _ptr(desc), _ptr(n),
                   _ptr(depth), F, rows, cols, cap, int(out_cap), *RGBD_FRAME.ptrs(out))
        return out

    def f2f_assemble_central(self, frames, ref_frame, cur_frame, keys, order, corr_cap, pct_good_matches=1.0,
                             max_hdiff=-1.0, out=None):
        """TrackerRGBDSE3.track_frame steps 1-2, batched.  frames: dict from rgbd_assemble; ref_frame / cur_frame
        [NP] i32; keys [NP, frame_cap, 1] u32, order [NP, frame_cap] i32 -> dict(f, p [NP,corr_cap,3] f64,
        q, t [NP,corr_cap] i32, n [NP] i32)."""
        NP = ref_frame.shape[0]
        frame_cap = frames["m"].shape[1]
        _check(ref_frame, torch.int32, "ref_frame", (NP,))
        _check(cur_frame, torch.int32, "cur_frame", (NP,))
        _check(keys, torch.uint32, "keys", (NP, frame_cap, 1))
        _check(order, torch.int32, "order", (NP, frame_cap))
        out = CORR_CENTRAL.of(ref_frame.device, out, NP=NP, cap=corr_cap)
        self._call(self._lib.sosvo_f2f_assemble_central, float(pct_good_matches), float(max_hdiff),
                   *RGBD_FRAME_READ.ptrs(frames), frame_cap, _ptr(ref_frame), _ptr(cur_frame), _ptr(keys), _ptr(order), NP,
                   int(corr_cap), *CORR_CENTRAL.ptrs(out))
        return out

    # ---- whole hot path ------------------------------------------------------------------
    def frame_pair_batch_workspace(self, cfg):
        return int(self._lib.sosvo_frame_pair_batch_workspace(_struct_ptr(cfg)))

    def frame_pair_batch_streams_workspace(self, cfg, n_streams):
        return int(self._lib.sosvo_frame_pair_batch_streams_workspace(_struct_ptr(cfg), int(n_streams)))

    def frame_pair_batch_join(self):
        """sosvo_frame_pair_batch_streams_join: the context's stream waits for every part of the latest enqueue."""
        self._call(self._lib.sosvo_frame_pair_batch_streams_join)

    def frame_pair_batch(self, rig, cfg, omni, unwrap_table, mask_bits, pattern, workspace, results=None, n_streams=1,
                         join=True):
        """omni [2B,H,W,3] u8, unwrap_table [2,rows,cols,2] u32, mask_bits [2,rows,cols] u32 (with SOSVO_FLAG_SEAM_FREE:
        cols + 80 columns, from unwrap_prepare_seam_free / mask_bits_seam_free), pattern [512,2] i8,
        workspace u8 [>= frame_pair_batch_workspace(cfg)] -> results [B,16] f64 (see include/sosvo.h).
        join=False (n_streams > 1 only): sosvo_frame_pair_batch_streams_enqueue -- call frame_pair_batch_join() before
        reading the records on this context's stream."""
        B = int(cfg.n_pairs)
        cols = _run_cols(cfg)
        _check(omni, torch.uint8, "omni", (2 * B, cfg.H, cfg.W, 3))
        _check(unwrap_table, torch.uint32, "unwrap_table", (2, cfg.rows, cols, 2))
        _check(mask_bits, torch.uint32, "mask_bits", (2, cfg.rows, cols))
        _check(pattern, torch.int8, "pattern", (512, 2))
        _check(workspace, torch.uint8, "workspace", ndim=1)
        results = _buf(results, torch.float64, "results", (B, 16), omni.device)
        if int(n_streams) > 1:   # the batch split over internal HIP streams of the library
            fn = self._lib.sosvo_frame_pair_batch_streams if join else self._lib.sosvo_frame_pair_batch_streams_enqueue
            self._call(fn, _struct_ptr(rig),
                       _struct_ptr(cfg), int(n_streams), _ptr(omni), _ptr(unwrap_table), _ptr(mask_bits),
                       _ptr(pattern), _ptr(workspace), int(workspace.numel()), _ptr(results))
            return results
        self._call(self._lib.sosvo_frame_pair_batch, _struct_ptr(rig),
                   _struct_ptr(cfg), _ptr(omni), _ptr(unwrap_table), _ptr(mask_bits), _ptr(pattern),
                   _ptr(workspace), int(workspace.numel()), _ptr(results))
        return results

    # ---- sequence mode, one or several sequences through one store (include/sosvo.h "Sequence mode", "Several sequences
    # through one frame store").  One helper per operation serves both families: `prefix` is "sosvo_sequence_" or
    # "sosvo_rgbd_sequence_", `heads` the structs the entry point takes first (rig or cam, cfg).
    @staticmethod
    def _host_ints(values, ctype=ctypes.c_int32):
        """Host ints as a C array behind a void* (never empty: an empty list is no null pointer); seeds wrap to 64 bits."""
        wrap = 2 ** 64 - 1 if ctype is ctypes.c_uint64 else -1   # (x & -1 == x)
        return ctypes.cast((ctype * max(len(values), 1))(*[int(x) & wrap for x in values]), c_p)

    def _seq_call(self, name, heads, window, slots, *args):
        self._call(getattr(self._lib, name), *[_struct_ptr(h) for h in heads], int(window), int(slots), *args)

    def _seq_workspace(self, prefix, cfg, window, slots):
        return int(getattr(self._lib, prefix + "workspace")(_struct_ptr(cfg), int(window), int(slots)))

    def _seq_front_end(self, prefix, heads, window, slots, images, first_slot, slot_of_frame, consts, workspace):
        """images: the tensors with one row per frame, consts: the model's; slot_of_frame None: ..._front_end at first_slot."""
        n = int(images[0].shape[0])
        if slot_of_frame is None:
            name, where = "front_end", int(first_slot)
        else:
            if len(slot_of_frame) != n:
                raise SosvoError("slot_of_frame: one slot per frame")
            name, where = "front_end_slots", self._host_ints(slot_of_frame)
        self._seq_call(prefix + name, heads, window, slots, *[_ptr(t) for t in images], n, where, *[_ptr(t) for t in consts],
                       _ptr(workspace), int(workspace.numel()))

    def _seq_track(self, prefix, heads, window, slots, ref_slots, cur_slots, seed, seeds, workspace, results):
        """seeds None: ..._track with the scalar seed; else ..._track_seeds."""
        n = len(ref_slots)
        if seeds is None and len(cur_slots) != n:
            raise SosvoError("ref_slots and cur_slots must have the same length")
        if seeds is not None and (len(cur_slots) != n or len(seeds) != n):
            raise SosvoError("ref_slots, cur_slots and seeds must have the same length")
        _check(workspace, torch.uint8, "workspace", ndim=1)
        _check(results, torch.float64, "results", (None, 16))
        if results.shape[0] < n:
            raise SosvoError("results holds fewer rows than slot pairs")
        name, tail = ("track", (n, int(seed))) if seeds is None else ("track_seeds", (self._host_ints(seeds, ctypes.c_uint64), n))
        self._seq_call(prefix + name, heads, window, slots, self._host_ints(ref_slots), self._host_ints(cur_slots), *tail,
                       _ptr(workspace), int(workspace.numel()), _ptr(results))
        return results

    def _seq_copy(self, prefix, cfg, window, slots, src, dst, workspace, lists):
        """lists False: ..._copy_slot of two ints; True: ..._copy_slots of two host sequences."""
        if not lists:
            args = ("copy_slot", int(src), int(dst))
        elif len(src) != len(dst):
            raise SosvoError("src_slots and dst_slots must have the same length")
        else:
            args = ("copy_slots", self._host_ints(src), self._host_ints(dst), len(src))
        self._seq_call(prefix + args[0], (cfg,), window, slots, *args[1:], _ptr(workspace), int(workspace.numel()))

    def _seq_counts(self, prefix, cfg, window, slots, first_slot, n, workspace):
        out = (ctypes.c_int32 * max(int(n), 1))()
        self._seq_call(prefix + "frame_counts", (cfg,), window, slots, int(first_slot), int(n), _ptr(workspace),
                       int(workspace.numel()), ctypes.cast(out, c_p))
        return [int(out[i]) for i in range(int(n))]

    @staticmethod
    def _check_omni_inputs(cfg, omni, unwrap_table, mask_bits, pattern, workspace):
        cols = _run_cols(cfg)
        _check(omni, torch.uint8, "omni", (None, cfg.H, cfg.W, 3))
        _check(unwrap_table, torch.uint32, "unwrap_table", (2, cfg.rows, cols, 2))
        _check(mask_bits, torch.uint32, "mask_bits", (2, cfg.rows, cols))
        _check(pattern, torch.int8, "pattern", (512, 2))
        _check(workspace, torch.uint8, "workspace", ndim=1)

    @staticmethod
    def _check_rgbd_inputs(cfg, bgr, depth, mask_bits, pattern, workspace):
        _check(bgr, torch.uint8, "bgr", (None, cfg.rows, cfg.cols, 3))
        _check(depth, torch.float32, "depth", (bgr.shape[0], cfg.rows, cfg.cols))
        _check(mask_bits, torch.uint32, "mask_bits", (1, cfg.rows, cfg.cols))
        _check(pattern, torch.int8, "pattern", (512, 2))
        _check(workspace, torch.uint8, "workspace", ndim=1)

    def sequence_workspace(self, cfg, window, slots):
        return self._seq_workspace("sosvo_sequence_", cfg, window, slots)

    def sequence_front_end(self, rig, cfg, window, slots, omni, first_slot, unwrap_table, mask_bits, pattern, workspace):
        """omni [n,H,W,3] u8 (n <= window) -> store slots first_slot .. first_slot + n - 1 (asynchronous)."""
        self._check_omni_inputs(cfg, omni, unwrap_table, mask_bits, pattern, workspace)
        self._seq_front_end("sosvo_sequence_", (rig, cfg), window, slots, (omni,), first_slot, None,
                            (unwrap_table, mask_bits, pattern), workspace)

    def sequence_track(self, rig, cfg, window, slots, ref_slots, cur_slots, seed, workspace, results):
        """ref_slots / cur_slots: host int sequences of equal length n <= cfg.n_pairs -> results[:n] [n,16] f64 (device,
        asynchronous); pair i samples with seed + i."""
        return self._seq_track("sosvo_sequence_", (rig, cfg), window, slots, ref_slots, cur_slots, seed, None, workspace, results)

    def sequence_copy_slot(self, cfg, window, slots, src, dst, workspace):
        self._seq_copy("sosvo_sequence_", cfg, window, slots, src, dst, workspace, False)

    def sequence_frame_counts(self, cfg, window, slots, first_slot, n, workspace):
        """-> list of n ints (StereoPanoramicFrame.num_valid_keypoints of the slots); synchronises the stream."""
        return self._seq_counts("sosvo_sequence_", cfg, window, slots, first_slot, n, workspace)

    def sequence_front_end_slots(self, rig, cfg, window, slots, omni, slot_of_frame, unwrap_table, mask_bits, pattern, workspace):
        """sequence_front_end with frame i's record written to store slot slot_of_frame[i] (host ints, one per frame of
        omni, no slot twice); asynchronous."""
        self._check_omni_inputs(cfg, omni, unwrap_table, mask_bits, pattern, workspace)
        self._seq_front_end("sosvo_sequence_", (rig, cfg), window, slots, (omni,), None, slot_of_frame,
                            (unwrap_table, mask_bits, pattern), workspace)

    def sequence_track_seeds(self, rig, cfg, window, slots, ref_slots, cur_slots, seeds, workspace, results):
        """sequence_track with pair i sampling with seeds[i] (host ints) -> results[:n] (device, asynchronous)."""
        return self._seq_track("sosvo_sequence_", (rig, cfg), window, slots, ref_slots, cur_slots, None, seeds, workspace, results)

    def sequence_copy_slots(self, cfg, window, slots, src_slots, dst_slots, workspace):
        """Store slots src_slots[i] -> dst_slots[i], all pairs in one launch (no slot written twice or read and written)."""
        self._seq_copy("sosvo_sequence_", cfg, window, slots, src_slots, dst_slots, workspace, True)

    def rgbd_sequence_workspace(self, cfg, window, slots):
        return self._seq_workspace("sosvo_rgbd_sequence_", cfg, window, slots)

    def rgbd_sequence_front_end(self, cam, cfg, window, slots, bgr, depth, first_slot, mask_bits, pattern, workspace):
        self._check_rgbd_inputs(cfg, bgr, depth, mask_bits, pattern, workspace)
        self._seq_front_end("sosvo_rgbd_sequence_", (cam, cfg), window, slots, (bgr, depth), first_slot, None,
                            (mask_bits, pattern), workspace)

    def rgbd_sequence_track(self, cfg, window, slots, ref_slots, cur_slots, seed, workspace, results):
        return self._seq_track("sosvo_rgbd_sequence_", (cfg,), window, slots, ref_slots, cur_slots, seed, None, workspace, results)

    def rgbd_sequence_copy_slot(self, cfg, window, slots, src, dst, workspace):
        self._seq_copy("sosvo_rgbd_sequence_", cfg, window, slots, src, dst, workspace, False)

    def rgbd_sequence_frame_counts(self, cfg, window, slots, first_slot, n, workspace):
        return self._seq_counts("sosvo_rgbd_sequence_", cfg, window, slots, first_slot, n, workspace)

    def rgbd_sequence_front_end_slots(self, cam, cfg, window, slots, bgr, depth, slot_of_frame, mask_bits, pattern, workspace):
        self._check_rgbd_inputs(cfg, bgr, depth, mask_bits, pattern, workspace)
        self._seq_front_end("sosvo_rgbd_sequence_", (cam, cfg), window, slots, (bgr, depth), None, slot_of_frame,
                            (mask_bits, pattern), workspace)

    def rgbd_sequence_track_seeds(self, cfg, window, slots, ref_slots, cur_slots, seeds, workspace, results):
        return self._seq_track("sosvo_rgbd_sequence_", (cfg,), window, slots, ref_slots, cur_slots, None, seeds, workspace, results)

    def rgbd_sequence_copy_slots(self, cfg, window, slots, src_slots, dst_slots, workspace):
        self._seq_copy("sosvo_rgbd_sequence_", cfg, window, slots, src_slots, dst_slots, workspace, True)

    def rgbd_pair_batch_workspace(self, cfg):
        return int(self._lib.sosvo_rgbd_pair_batch_workspace(_struct_ptr(cfg)))

    def rgbd_pair_batch(self, cam, cfg, bgr, depth, mask_bits, pattern, workspace, results=None):
        """bgr [2B,rows,cols,3] u8, depth [2B,rows,cols] f32, mask_bits [1,rows,cols] u32, pattern [512,2] i8,
        workspace u8 [>= rgbd_pair_batch_workspace(cfg)] -> results [B,16] f64 (see include/sosvo.h)."""
        B = int(cfg.n_pairs)
        _check(bgr, torch.uint8, "bgr", (2 * B, cfg.rows, cfg.cols, 3))
        _check(depth, torch.float32, "depth", (2 * B, cfg.rows, cfg.cols))
        _check(mask_bits, torch.uint32, "mask_bits", (1, cfg.rows, cfg.cols))
        _check(pattern, torch.int8, "pattern", (512, 2))
        _check(workspace, torch.uint8, "workspace", ndim=1)
        results = _buf(results, torch.float64, "results", (B, 16), bgr.device)
        self._call(self._lib.sosvo_rgbd_pair_batch, _struct_ptr(cam),
                   _struct_ptr(cfg), _ptr(bgr), _ptr(depth), _ptr(mask_bits), _ptr(pattern),
                   _ptr(workspace), int(workspace.numel()), _ptr(results))
        return results

    def f2f_assemble(self, rig, frames, ref_frame, cur_frame, keys_top, order_top, keys_bot, order_bot, corr_cap,
                     out=None, cyclic=False):
        """frames = dict from stereo_assemble; ref_frame / cur_frame [NP] i32; keys_* [NP, frame_cap, 1] u32,
        order_* [NP, frame_cap] i32 -> dict(f, p [NP,corr_cap,3] f64, cam, q, t [NP,corr_cap] i32, n, n_top [NP]).  cyclic:
        sosvo_f2f_assemble_cyclic, the |du| gate around the circle (period = the rig's pano_top[0] / pano_bot[0])."""
        F, frame_cap = frames["m_top"].shape[0], frames["m_top"].shape[1]
        NP = ref_frame.shape[0]
        _check(ref_frame, torch.int32, "ref_frame", (NP,))
        _check(cur_frame, torch.int32, "cur_frame", (NP,))
        FRAME_MATCHED.check(frames, F=F, cap=frame_cap)
        for name, t in (("keys_top", keys_top), ("keys_bot", keys_bot)):
            _check(t, torch.uint32, name, (NP, frame_cap, 1))
        for name, t in (("order_top", order_top), ("order_bot", order_bot)):
            _check(t, torch.int32, name, (NP, frame_cap))
        out = CORR.of(ref_frame.device, out, NP=NP, cap=corr_cap)
        self._call(self._lib.sosvo_f2f_assemble_cyclic if cyclic else self._lib.sosvo_f2f_assemble, _struct_ptr(rig),
                   *FRAME_MATCHED.ptrs(frames), frame_cap, _ptr(ref_frame), _ptr(cur_frame), _ptr(keys_top), _ptr(order_top),
                   _ptr(keys_bot), _ptr(order_bot), NP, corr_cap, *CORR.ptrs(out))
        return out
