"""Batched image front end: omni frames -> per-bucket keypoints + descriptors of both panoramas, i.e.
OmniStereoModel.set_current_omni_image (omnistereo/camera_models.py:3107-3120) followed by
OmniCamModel.detect_sparse_features_on_panorama for both mirrors (camera_models.py:1610-1797), for F frames
at once.  All buffers live in HBM; a run is five asynchronous C-ABI calls (K1, K2+K3, K4, K6)."""
import numpy as np
import torch

from . import _lib, orb_pattern
from .device import DETECTED, ORB, ORB_DESC, Context


class DeviceImageModel(object):
    """Per-model constants of the image stages, uploaded once: float32 unwrap maps and annulus masks of the two
    mirrors, the azimuthal masks as bit fields, the descriptor pattern."""

    def __init__(self, ctx, gums, omni_shape, azimuth_mask_degrees=30, overlap_degrees=0, elev_mask_padding=10,
                 stand_masks_azimuth_coord_in_degrees_list=(50, 170, 290), stand_masks_width_in_degrees=10,
                 mask_bits=None):
        """Defaults are TrackerStereoSE3.bootstrap_tracker's (pose_est_tools.py:870-878).  `mask_bits`
        [2, rows, cols] uint32 may be given to skip the mask construction."""
        assert isinstance(ctx, Context)
        top, bot = gums.top_model, gums.bot_model
        if top.mask is None or bot.mask is None:
            gums.make_annulus_masks(omni_shape)
        self.H, self.W = omni_shape
        self.rows, self.cols = top.panorama.rows, top.panorama.cols
        assert (bot.panorama.rows, bot.panorama.cols) == (self.rows, self.cols)
        maps = [m.panorama.float32_maps() for m in (top, bot)]
        dev = ctx.device
        self.map_x = torch.from_numpy(np.stack([maps[0][0], maps[1][0]])).to(dev)
        self.map_y = torch.from_numpy(np.stack([maps[0][1], maps[1][1]])).to(dev)
        self.omni_masks = torch.from_numpy(np.stack([top.mask, bot.mask])).to(dev)
        if mask_bits is None:
            bits = []
            for m in (top, bot):
                m.panorama.generate_azimuthal_masks(
                    azimuth_mask_degrees, overlap_degrees, elev_mask_padding=elev_mask_padding,
                    stand_masks_azimuth_coord_in_degrees_list=list(stand_masks_azimuth_coord_in_degrees_list),
                    stand_masks_width_in_degrees=stand_masks_width_in_degrees, omni_shape=omni_shape)
                bits.append(m.panorama.mask_bits())
            mask_bits = np.stack(bits)
            self.nmask = max(1, len(top.panorama.azimuthal_masks))
        else:
            self.nmask = int(np.log2(float(mask_bits.max()))) + 1 if mask_bits.max() > 0 else 1
        self.mask_bits_host = np.ascontiguousarray(mask_bits, dtype=np.uint32)
        self.mask_bits = torch.from_numpy(self.mask_bits_host).to(dev)
        self.pattern_host = orb_pattern.orb_pattern()
        self.pattern = torch.from_numpy(self.pattern_host).to(dev)
        self.seam_free, self.cols_run = False, self.cols     # (the plain form: the image stages run at the panorama's width)

    def seam_free_form(self, ctx):
        """The model as a seam-free front end sees it, made once: see SeamFreeImageModel."""
        if self.__dict__.get("_seam_free_form") is None:
            self._seam_free_form = SeamFreeImageModel(ctx, self)
        return self._seam_free_form


class SeamFreeImageModel(object):
    """A DeviceImageModel for the seam-free front end: the image stages run on panoramas padded by SEAM_HALO cyclic columns on
    either side, `cols_run` = cols + 80 wide.  `unwrap_table_run` [2, rows, cols_run, 2] and `mask_bits_run` [2, rows, cols_run]
    (the masks with an empty halo) are made on the device; every plain member (cols: the period, mask_bits, unwrap_table, ...)
    is the plain model's, unchanged for its other users."""
    seam_free = True

    def __init__(self, ctx, model):
        _lib.seam_free_check(model.cols)
        self.plain, self.cols_run = model, model.cols + 2 * _lib.SEAM_HALO
        self.unwrap_table_run = ctx.unwrap_prepare_seam_free(model.omni_masks, model.map_x, model.map_y, (model.H, model.W))
        self.mask_bits_run = ctx.mask_bits_seam_free(model.mask_bits)
        ctx.synchronize()      # (front ends on other streams that share the model find them ready)

    def seam_free_form(self, ctx):
        return self

    def __getattr__(self, name):    # (only what this form does not have itself)
        return getattr(self.__dict__["plain"], name)


def default_kp_cap(method, num_of_features):
    """ImageFrontEnd's keypoint capacity per (frame, mirror, mask) when none is given (also the batched engines')."""
    method = str(method).upper()
    if method in ("FAST", "AGAST"):  # every corner is kept (num_of_features only names the ORB descriptor object)
        return 2048
    if method == "ORB":  # retainBest keeps ties beyond the quota: leave head room
        return int(min(2048, max(64, -(-int(num_of_features * 1.25) // 64) * 64)))
    return int(min(1024, max(64, -(-int(num_of_features) // 64) * 64)))


def mirror_kp_cap(method, num_of_features):
    """The per-frame mirror path's capacity (GUMStereo._front_end): what a batched engine must use to compute what
    StereoPanoramicFrame computes (FAST / AGAST keep the first `cap` corners in raster order, and ORB's retainBest
    head room changes the output)."""
    scale = 1.25 if str(method).upper() == "ORB" else 1.0
    return int(min(4096, max(64, -(-int(num_of_features * scale) // 64) * 64)))


class ImageFrontEnd(object):
    def __init__(self, ctx, model, nframes, detection_method="GFT", num_of_features=1000, kp_cap=None,
                 median_win_size=11, quality=0.01, min_distance=5.0, edge=31, keep_panoramas=True,
                 skip_unreachable_rows=True, subpix=None):
        """model: a DeviceImageModel, or its seam_free_form(ctx) for the seam-free front end (gray and
        panoramas are cols + 80 wide, keypoints are in the padded columns until unpad(); ORB and edge > 31 are refused).
        num_of_features: per azimuthal mask (FeatureMatcher.num_of_features, pose_est_tools.py:862).
        keep_panoramas=False: K1 is fused into the median kernel and the colour panoramas are not materialised
        (nothing downstream of K3 reads them); identical gray images.
        subpix: None = off, or the window half-size 2 .. 5 of the sub-pixel refinement (Context.refine_subpix) that
        run_features applies to the keypoints after their descriptors are computed."""
        if detection_method.upper() not in ("GFT", "ORB", "FAST", "AGAST"):
            raise NotImplementedError("detection method %r: GFT (the reference default, pose_est_tools.py:684), ORB, "
                                      "FAST and AGAST are built" % detection_method)
        self.ctx, self.model, self.F = ctx, model, int(nframes)
        self.method = detection_method.upper()
        self.num_of_features, self.median_win_size = int(num_of_features), int(median_win_size)
        self.quality, self.min_distance, self.edge = float(quality), float(min_distance), int(edge)
        self.skip_unreachable_rows = bool(skip_unreachable_rows)
        self.subpix = _lib.subpix_half(subpix)
        self.kp_cap = int(kp_cap) if kp_cap else default_kp_cap(self.method, self.num_of_features)
        self.seam_free = bool(getattr(model, "seam_free", False))
        if self.seam_free:
            _lib.seam_free_check(model.cols, self.method, self.edge)
        dev, m = ctx.device, model
        cols = m.cols_run if self.seam_free else m.cols
        NI, P = 2 * self.F, 2 * self.F * m.nmask
        self.omni = torch.zeros((self.F, m.H, m.W, 3), dtype=torch.uint8, device=dev)
        self.keep_panoramas = bool(keep_panoramas) or self.median_win_size not in (0, 1, 3, 5, 11)
        self.pano = torch.zeros((2, self.F, m.rows, cols, 3), dtype=torch.uint8, device=dev) if self.keep_panoramas else None
        self.gray = torch.zeros((NI, m.rows, cols), dtype=torch.uint8, device=dev)
        self.kp, self.n, self.status = DETECTED.alloc(dev, zeroed=True, P=P, cap=self.kp_cap).values()
        self.desc = ORB_DESC.alloc(dev, zeroed=True, P=P, cap=self.kp_cap)["desc"]
        self.cos_a, self.sin_a = orb_pattern.angle_cos_sin(orb_pattern.GFT_KEYPOINT_ANGLE)
        # Rows no consumer can reach (beyond the masks' elevation padding + the GFT halo and the descriptor border) are
        # not computed by the fused K1-K3 kernel.  Model constant, keyed by what it depends on; computed here (and
        # waited for) so that front ends on other streams that share the model find it ready.
        self.gray_rows = None
        if self.method == "GFT" and skip_unreachable_rows and not self.keep_panoramas:
            key = (self.edge, self.cos_a, self.sin_a)
            cache = m.__dict__.setdefault("_gray_rows", {})
            if key not in cache:
                cache[key] = ctx.gray_rows_needed(self._mask_bits, m.nmask, self.edge, m.pattern, self.cos_a, self.sin_a)
                ctx.synchronize()
            self.gray_rows = cache[key]
        if self.method == "ORB":
            self.kp4, self.resp = ORB.sub("kp4", "resp").alloc(dev, zeroed=True, P=P, cap=self.kp_cap).values()
            if getattr(model, "mask_pyr", None) is None:
                model.mask_pyr = ctx.orb_mask_pyramid(model.mask_bits, model.nmask)

    @property
    def _mask_bits(self):
        """The mask bits the detectors run on: the model's, or (seam-free) those with the empty halo."""
        return self.model.mask_bits_run if self.seam_free else self.model.mask_bits

    def load_frames(self, omni):
        """omni: numpy or torch uint8 [F, H, W, 3] (BGR) -> resident in HBM."""
        t = torch.from_numpy(np.ascontiguousarray(omni)) if isinstance(omni, np.ndarray) else omni
        self.omni.copy_(t.to(self.ctx.device))

    def run(self, unpad=True):
        """unpad=False: a seam-free front end leaves its keypoints in the padded columns (the pair pipeline's static stereo
        reads the padded gray around them and calls unpad() itself)."""
        self.run_images()
        self.run_features()
        if self.seam_free and unpad:
            self.unpad()

    def unpad(self):
        """Seam-free: the keypoints of both views from the padded columns back to the period's (Context.keypoints_unpad)."""
        self.ctx.keypoints_unpad(self.kp, self.n, self.model.cols)

    def gray_interior(self, out=None):
        """Seam-free: the gray panoramas at the period's width [2 F, rows, cols] (Context.gray_unpad), for what reads them as a
        circle (the cyclic pyramid of the Lucas-Kanade tracker)."""
        return self.ctx.gray_unpad(self.gray, self.model.cols, row_range=None if self.keep_panoramas else self.gray_rows, out=out)

    def run_images(self):
        """K1 + K2 + K3: omni frames -> median-blurred gray panoramas (the VALU-bound half of the front end)."""
        c, m = self.ctx, self.model
        if self.seam_free:
            table, cols = m.unwrap_table_run, m.cols_run
        else:
            if getattr(m, "unwrap_table", None) is None:  # once per model
                m.unwrap_table = c.unwrap_prepare(m.omni_masks, m.map_x, m.map_y, (m.H, m.W))
            table, cols = m.unwrap_table, m.cols
        if self.keep_panoramas:
            c.unwrap_table(self.omni, table, pano=self.pano)                                          # K1 (a1 + a2)
            c.median_gray(self.pano.view(2 * self.F, m.rows, cols, 3), self.median_win_size, gray=self.gray)  # K2 + K3
        else:
            c.unwrap_median_gray(self.omni, table, self.median_win_size, gray=self.gray,
                                 row_range=self.gray_rows)                                           # K1 + K2 + K3

    def run_features(self):
        """K4 / K5 + K6: keypoints and descriptors per azimuthal mask on the gray panoramas; then, with `subpix`, the
        keypoints move to their sub-pixel positions (the descriptors stay those of the detector's positions)."""
        self._detect_describe()
        if self.subpix is not None:
            self.ctx.refine_subpix(self.gray, self.kp, self.n, self.model.nmask, half=self.subpix,
                                   row_range=None if self.keep_panoramas else self.gray_rows)

    def _detect_describe(self):
        c, m = self.ctx, self.model
        if self.method == "ORB":
            c.detect_describe_orb(self.gray, m.mask_pyr, self.F, m.nmask, self.num_of_features, m.pattern, self.kp4,
                                  self.resp, self.n, self.desc, kp_xy=self.kp)                   # K5 + K6' on one pyramid
            return
        if self.method in ("FAST", "AGAST"):
            (c.detect_fast if self.method == "FAST" else c.detect_agast)(
                self.gray, self._mask_bits, self.F, m.nmask, self.kp_cap, threshold=10, kp=self.kp, n=self.n,
                status=self.status)                                                               # FAST / AGAST + NMS
            c.describe_orb(self.gray, self.kp, self.n, m.nmask, m.pattern, self.cos_a, self.sin_a, edge=self.edge,
                           desc=self.desc)                                                        # K6
            return
        c.detect_gft(self.gray, self._mask_bits, self.F, m.nmask, self.kp_cap, quality=self.quality,
                     min_distance=self.min_distance, max_corners=self.num_of_features, kp=self.kp, n=self.n,
                     status=self.status)                                                          # K4
        c.describe_orb(self.gray, self.kp, self.n, m.nmask, m.pattern, self.cos_a, self.sin_a, edge=self.edge,
                       desc=self.desc, row_range=None if self.keep_panoramas else self.gray_rows)  # K6

    # views in the layout the matching stages expect: problem = frame * nmask + mask
    def view_arrays(self):
        h = self.F * self.model.nmask
        return dict(kp_top=self.kp[:h], kp_bot=self.kp[h:], desc_top=self.desc[:h], desc_bot=self.desc[h:],
                    n_top=self.n[:h], n_bot=self.n[h:])
