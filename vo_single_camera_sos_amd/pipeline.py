"""Batched frame-pair front end: the order of operations of one reference VO step
(StereoPanoramicFrame.__init__ -> TrackerStereoSE3.track_frame, omnistereo/pose_est_tools.py:271-402,
:736-847) for B independent frame pairs at once, every buffer resident in HBM, every stage one or two
asynchronous C-ABI calls on one stream, no host synchronisation inside a step.

Pair i tracks frame 2i+1 (current) against frame 2i (reference / keyframe)."""
import threading

import numpy as np
import torch

from ._lib import LK_MAX_LEVELS, SEAM_FREE, StepOptions, cyclic_value, detector_code, rgbd_detector_flags
from .device import CORR, CORR_CENTRAL, DETECTED, FRAME, ORB, ORB_DESC, RANSAC, RGBD_FRAME, Context, make_rig


class RigConfig(object):
    """What the hot path needs to know about one calibrated omnistereo rig (host numbers)."""

    def __init__(self, pano_top, pano_bot, F_top, F_bot, min_range, max_range, stereo_min_disp=1.0,
                 stereo_max_hdiff=2.5, f2f_max_hdiff=None, pct_good_matches=1.0):
        self.pano_top, self.pano_bot = tuple(pano_top), tuple(pano_bot)
        self.F_top, self.F_bot = np.asarray(F_top, np.float64), np.asarray(F_bot, np.float64)
        self.min_range, self.max_range = float(min_range), float(max_range)
        self.stereo_min_disp, self.stereo_max_hdiff = float(stereo_min_disp), float(stereo_max_hdiff)
        # TrackerStereoSE3.bootstrap_tracker (pose_est_tools.py:866): 0.125 * 0.5 * pano cols
        self.f2f_max_hdiff = 0.125 * 0.5 * self.pano_top[0] if f2f_max_hdiff is None else float(f2f_max_hdiff)
        self.pct_good_matches = float(pct_good_matches)

    def as_struct(self):
        return make_rig(self.pano_top, self.pano_bot, self.F_top, self.F_bot, self.min_range, self.max_range,
                        self.stereo_min_disp, self.stereo_max_hdiff, self.f2f_max_hdiff, self.pct_good_matches)


class FramePairPipeline(object):
    def __init__(self, ctx, rig, n_pairs, nmask=12, bucket_cap=192, frame_cap=2048, thr=None, max_iter=2000,
                 adaptive=False, seed=0, lm_iter=30, front_end=None, ransac_solver="P3P", cross_check_stereo=False,
                 cross_check_f2f=False, gated_stereo=False, gated_f2f=False, gated_max_distance=None, ratio_stereo=False,
                 ratio_f2f=False, ratio=None, subpix=None, f2f_tracker="match", lk=None, stereo_refine=None, stereo_lk=None,
                 cyclic_columns=False):
        """front_end: an ImageFrontEnd over 2 * n_pairs frames; its keypoint/descriptor buffers are used in
        place (no copy).  Without it, keypoints are loaded with load_keypoints().
        ransac_solver: "GP3P" = generalised P3P on samples across both mirrors (what the reference's non-central RANSAC
        uses, pose_est_tools.py:696); "P3P" = the three solve points of a sample from one mirror (BASELINE config 2).
        cross_check_stereo / cross_check_f2f: mutual matches only (cv2.BFMatcher's crossCheck, camera_models.py:401) in
        the static-stereo matcher / the frame-to-frame matcher.
        gated_stereo / gated_f2f: the matcher searches among the candidates that pass the stage's own pixel gate
        (Context.match_hamming_gated); gated_max_distance: None = no cap, or 1 .. 256: a match whose Hamming distance
        exceeds it is no match.
        ratio_stereo / ratio_f2f: Lowe's ratio rule fused into that matcher's search (Context.match_hamming_ratio), plain or
        under the gate; ratio: a float in (0, 1) with ratio * 64 an integer (0.75 = the reference's, camera_models.py:423).
        subpix: None = the front end's own setting, or the window half-size 2 .. 5 of the sub-pixel keypoint refinement,
        handed on to the front end (ImageFrontEnd's subpix).
        f2f_tracker: "match" = the frame-to-frame correspondences come from the descriptor matcher (the reference's way);
        "lk" = the reference frames' stereo points are tracked into the current frames' gray panoramas by pyramidal
        Lucas-Kanade (Context.track_lk; cv2.calcOpticalFlowPyrLK, camera_models.py:3070) -- needs a front end.  lk: its
        settings, None / an LKOptions / a dict of its fields (half, levels, max_iter, eps, min_eig, fb_max).
        stereo_refine: None, or "lk" = sub-pixel static stereo: between sort_matches and stereo_assemble the bottom keypoint of
        every matched pair is tracked from the top panorama into the bottom one (Context.refine_stereo_lk; the same call of
        the reference, between the two views of one frame) -- needs a front end.  stereo_lk: its settings, None / a
        StereoLKOptions / a dict of its fields (half, max_iter, eps, min_eig, max_shift).
        cyclic_columns: the panoramas are full circles, column `cols` is column 0 again: the
        frame-to-frame |du| gate is cyclic in the assemble and, with gated_f2f, inside the matcher; with f2f_tracker="lk" the
        pyramids and the tracker are cyclic too (cols a multiple of 2^(levels - 1), the top level at least 2 half + 3 columns
        wide).  The period is the rig's pano_top[0] / pano_bot[0].  "seam_free": all of that plus the seam-free front end
         -- front_end is an ImageFrontEnd over the model's seam_free_form(ctx); its keypoints stay in the
        padded columns through the static-stereo matching and refinement and are unpadded before the stereo assemble (a refined
        pair that ends up straddling the seam fails the plain stereo gate and is dropped); the tracker's cyclic pyramid is built
        on the interior columns (Context.gray_unpad)."""
        assert isinstance(ctx, Context)
        # (ValueError for a value out of range, settings without their switch, a width that cannot be cyclic, what reads the gray
        # panoramas without a front end.  This tracker has never refused the options of the matcher it replaces)
        so = StepOptions.of(cross_check_stereo, cross_check_f2f, gated_stereo, gated_f2f, gated_max_distance, ratio_stereo,
                            ratio_f2f, ratio, subpix, f2f_tracker, lk, stereo_refine, stereo_lk, cyclic_columns, rig,
                            order=StepOptions.PAIR_ORDER, tracker_sees_match=False, gray=front_end is not None,
                            detection_method=getattr(front_end, "method", "GFT"), edge=getattr(front_end, "edge", 31))
        if so.seam_free != bool(getattr(front_end, "seam_free", False)):
            raise ValueError("cyclic_columns=\"seam_free\" and a front end over the model's seam_free_form(ctx) go together")
        self.opts = o = so.match
        self.lk, self.stereo_lk, self.cyclic, self.f2f_tracker = so.lk, so.stereo_lk, so.cyclic, f2f_tracker
        if subpix is not None:
            front_end.subpix = so.subpix
        self.ctx, self.rig_cfg, self.rig = ctx, rig, rig.as_struct()
        self.front_end = front_end
        if front_end is not None:
            assert front_end.F == 2 * int(n_pairs)
            nmask, bucket_cap = front_end.model.nmask, front_end.kp_cap
        self.B, self.F, self.NM = int(n_pairs), 2 * int(n_pairs), int(nmask)
        self.bucket_cap, self.frame_cap, self.corr_cap = int(bucket_cap), int(frame_cap), 2 * int(frame_cap)
        # TrackerSE3.set_global_parameters_for_tracking (pose_est_tools.py:675-676)
        self.thr = float(1.0 - np.cos(np.deg2rad(5.0))) if thr is None else float(thr)
        self.max_iter, self.adaptive, self.seed, self.lm_iter = int(max_iter), bool(adaptive), int(seed), int(lm_iter)
        if str(ransac_solver).upper() not in ("P3P", "GP3P"):
            raise ValueError("ransac_solver: P3P or GP3P")
        self.gp3p = str(ransac_solver).upper() == "GP3P"
        dev = ctx.device
        P = self.F * self.NM
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        if front_end is not None:
            v = front_end.view_arrays()
            self.kp_top, self.kp_bot, self.desc_top, self.desc_bot = v["kp_top"], v["kp_bot"], v["desc_top"], v["desc_bot"]
            self.n_top, self.n_bot = v["n_top"], v["n_bot"]
        else:
            self.kp_top, self.kp_bot = z((P, bucket_cap, 2), torch.float32), z((P, bucket_cap, 2), torch.float32)
            self.desc_top, self.desc_bot = z((P, bucket_cap, 32), torch.uint8), z((P, bucket_cap, 32), torch.uint8)
            self.n_top, self.n_bot = z((P,), torch.int32), z((P,), torch.int32)
        self.s_keys, self.s_order = z((P, bucket_cap, 1), torch.uint32), z((P, bucket_cap), torch.int32)
        self.s_keys_rev = z((P, bucket_cap, 1), torch.uint32) if o.cross_check_stereo else None
        self.s_rivals = z((P, bucket_cap, 1), torch.uint32) if o.ratio_stereo else None
        # what stereo() / track() hand the matching step: query = bottom, train = top under the gate of stereo_assemble; the
        # |du| gate of f2f_assemble
        self._stereo_search = dict(cross_check=o.cross_check_stereo, keys_rev=self.s_keys_rev, ratio_64ths=o.ratio_64ths_stereo,
                                   rivals=self.s_rivals, keys=self.s_keys,
                                   gate=(rig.stereo_min_disp, rig.stereo_max_hdiff, gated_max_distance) if o.gated_stereo else None)
        Fc, Cc = self.frame_cap, self.corr_cap
        # descriptors and counts of both views back to back (view-major): the two frame-to-frame matchings of a step
        # (top with top, bottom with bottom) are ONE launch of 2B problems, and so are the two sorts
        self._d2 = z((2, self.F, Fc, 32), torch.uint8)
        self._M2 = z((2, self.F), torch.int32)
        self._m2 = z((2, self.F, Fc, 2), torch.float32)      # (the positions likewise: the gated search reads them)
        self.frames = dict(m_top=self._m2[0], m_bot=self._m2[1], d_top=self._d2[0], d_bot=self._d2[1], M=self._M2[0],
                           **FRAME.sub("X", "b_top", "b_bot", "n_cand").alloc(dev, zeroed=True, F=self.F, cap=Fc))
        self.ref_frame = torch.arange(0, self.F, 2, dtype=torch.int32, device=dev)
        self.cur_frame = torch.arange(1, self.F, 2, dtype=torch.int32, device=dev)
        q = torch.cat([self.cur_frame, self.cur_frame + self.F])   # problem i: top view, B + i: bottom view
        t = torch.cat([self.ref_frame, self.ref_frame + self.F])
        self._o2 = z((2 * self.B, Fc), torch.int32)
        if o.cross_check_f2f:   # the 2B role-swapped problems ride in the same launch, after the 2B forward ones
            q, t = torch.cat([q, t]), torch.cat([t, q])
        self._q, self._t, self._k = q, t, z((len(q), Fc, 1), torch.uint32)
        self._q2, self._t2, self._k2 = q[: 2 * self.B], t[: 2 * self.B], self._k[: 2 * self.B]     # the forward problems
        self._f2f_search = dict(ratio_64ths=o.ratio_64ths_f2f, rivals=torch.zeros_like(self._k) if o.ratio_f2f else None,
                                gate=(-1.0, rig.f2f_max_hdiff, gated_max_distance) if o.gated_f2f else None)
        if self.cyclic and o.gated_f2f:    # (one search serves both views: StepOptions.of checked that their widths agree)
            self._f2f_search["period"] = float(rig.pano_top[0])
        self._cyc = dict(cyclic=True) if self.cyclic else {}     # (off: the assembles are called as they always were)
        self.k_top, self.k_bot = self._k2[: self.B], self._k2[self.B:]
        self.o_top, self.o_bot = self._o2[: self.B], self._o2[self.B:]
        self.corr = CORR.alloc(dev, zeroed=True, NP=self.B, cap=Cc)
        self.ransac = RANSAC.alloc(dev, zeroed=True, P=self.B, S=Cc)
        self.T = z((self.B, 3, 4), torch.float64)
        self.lm_cost, self.lm_iters = z((self.B,), torch.float64), z((self.B,), torch.int32)
        self.cam_off = torch.from_numpy(np.stack([rig.F_top, rig.F_bot])).to(dev)
        self.cam_rot = torch.from_numpy(np.stack([np.eye(3), np.eye(3)])).to(dev)
        if self.stereo_lk is not None:    # the refinement's flags, one per bottom keypoint
            self.s_lk_status = z((P, self.bucket_cap), torch.uint8)
        if self.lk is not None:    # the tracker's buffers: 2B problems (top views, then bottom views), frame_cap points each
            self._lk_pyr = None
            self._lk_prev = z((2 * self.B, Fc, 2), torch.float32)
            self._lk_n = z((2 * self.B,), torch.int32)
            self._lk_out = (z((2 * self.B, Fc, 2), torch.float32), z((2 * self.B, Fc), torch.uint8),
                            z((2 * self.B, Fc), torch.float32)) + \
                ((z((2 * self.B, Fc, 2), torch.float32),) if self.lk.fb_max is not None else ())
            self._lk_ref = self._t2.to(torch.int64)

    # ---- inputs ------------------------------------------------------------------------------
    def load_keypoints(self, packed):
        """Image-free entry: per-bucket keypoints/descriptors as numpy arrays (tests/synth.pack_buckets)."""
        dev = self.ctx.device
        for name in ("kp_top", "kp_bot", "desc_top", "desc_bot", "n_top", "n_bot"):
            getattr(self, name).copy_(torch.from_numpy(packed[name]).to(dev))

    # ---- one step ----------------------------------------------------------------------------
    def stereo(self):
        c = self.ctx
        c.match_1nn_two_launch(self.desc_bot, self.desc_top, self.n_bot, self.n_top, q_pos=self.kp_bot, t_pos=self.kp_top,
                               **self._stereo_search)
        c.sort_matches(self.s_keys, self.n_bot, order=self.s_order)
        if self.stereo_lk is not None:
            fe = self.front_end
            c.refine_stereo_lk(fe.gray, self.kp_top, self.n_top, self.kp_bot, self.n_bot, self.s_keys, self.NM,
                               self.rig_cfg.stereo_min_disp, self.rig_cfg.stereo_max_hdiff, stereo_lk=self.stereo_lk,
                               row_range=None if fe.keep_panoramas else fe.gray_rows, status=self.s_lk_status)
        if self.cyclic == SEAM_FREE:    # (everything above ran in the padded columns)
            self.front_end.unpad()
        c.stereo_assemble(self.rig, self.kp_top, self.kp_bot, self.desc_top, self.desc_bot, self.n_top, self.n_bot,
                          self.s_keys, self.s_order, self.F, self.NM, self.frame_cap, out=self.frames)

    def _track_lk(self):
        """The frame-to-frame correspondences by tracking: pyramids of the front end's gray panoramas, the reference frames'
        m_top / m_bot tracked into the current frames' images as ONE launch of 2B problems, the tracked assemble."""
        c, fe, o = self.ctx, self.front_end, self.lk
        self._M2[1].copy_(self._M2[0])
        rr = None if fe.keep_panoramas else fe.gray_rows
        gray = fe.gray
        if self.cyclic == SEAM_FREE:    # the circle is the interior of the padded panoramas
            gray = self._lk_gray = fe.gray_interior(out=getattr(self, "_lk_gray", None))
        self._lk_pyr = (c.gray_pyramid_cyclic if self.cyclic else c.gray_pyramid)(gray, o.levels, row_range=rr, out=self._lk_pyr)
        torch.index_select(self._m2.view(2 * self.F, self.frame_cap, 2), 0, self._lk_ref, out=self._lk_prev)
        torch.index_select(self._M2.view(2 * self.F), 0, self._lk_ref, out=self._lk_n)
        res = c.track_lk(self._lk_pyr, self._t2, self._q2, self._lk_prev, self._lk_n, half=o.half, max_iter=o.max_iter,
                         eps=o.eps, min_eig=o.min_eig, fb_max=o.fb_max, out=self._lk_out)
        nxt, st = res[0], res[1]
        c.f2f_assemble_tracked(self.rig, self.frames, self.ref_frame, nxt[: self.B], nxt[self.B:], st[: self.B], st[self.B:],
                               self.corr_cap, out=self.corr, **self._cyc)

    def track(self):
        c, fr = self.ctx, self.frames
        if self.lk is not None:
            self._track_lk()
            return self._solve()
        self._M2[1].copy_(self._M2[0])                      # the bottom view's blocks have the same counts
        d2, M2 = self._d2.view(2 * self.F, self.frame_cap, 32), self._M2.view(2 * self.F)
        m2 = self._m2.view(2 * self.F, self.frame_cap, 2)
        c.match_1nn_slots(d2, m2, M2, self._q, self._t, self._k, 2 * self.B, **self._f2f_search)   # both views, 2B problems
        c.sort_matches(self._k2, M2, order=self._o2, q_slot=self._q2)
        c.f2f_assemble(self.rig, fr, self.ref_frame, self.cur_frame, self.k_top, self.o_top, self.k_bot, self.o_bot,
                       self.corr_cap, out=self.corr, **self._cyc)
        self._solve()

    def _solve(self):
        c, co = self.ctx, self.corr
        c.ransac_abs_pose(co["f"], co["p"], co["n"], self.thr, self.max_iter, seed=self.seed, adaptive=self.adaptive,
                          cam=co["cam"], cam_off=self.cam_off, cam_rot=self.cam_rot, cam_rot_identity=True,
                          out=self.ransac, gp3p=self.gp3p)
        self.T.copy_(self.ransac["T"])
        c.refine_abs_pose(co["f"], co["p"], co["n"], self.T, idx=self.ransac["idx"], m=self.ransac["n_inliers"],
                          cam=co["cam"], cam_off=self.cam_off, cam_rot=self.cam_rot, max_lm_iter=self.lm_iter,
                          cost=self.lm_cost, iters=self.lm_iters)

    def step(self):
        """The whole hot path for all B pairs (asynchronous): image front end (when attached), stereo
        correspondences, frame-to-frame tracking."""
        if self.front_end is not None and self.cyclic == SEAM_FREE:
            self.front_end.run(unpad=False)     # (stereo() unpads, after its refinement)
        elif self.front_end is not None:
            self.front_end.run()
        self.stereo()
        self.track()
        return self.T

    def results(self, out=None):
        """[B,16] f64 rows: 3x4 refined pose, n_inliers, n_correspondences, status, RANSAC best iteration
        (the per-pair record gathered over ranks in the multi-GPU configuration)."""
        if out is None:
            out = torch.empty((self.B, 16), dtype=torch.float64, device=self.ctx.device)
        out[:, :12] = self.T.reshape(self.B, 12)
        out[:, 12] = self.ransac["n_inliers"].to(torch.float64)
        out[:, 13] = self.corr["n"].to(torch.float64)
        out[:, 14] = self.ransac["info"][:, 2].to(torch.float64)
        out[:, 15] = self.ransac["info"][:, 0].to(torch.float64)
        return out


class OverlappedFramePairs(object):
    """The hot path for B pairs split over S HIP streams (one libsosvo context, front end and pipeline per
    stream, model constants shared).  The path alternates between a VALU-bound stage (K1-K3, the median) and
    latency-bound ones (corner selection, descriptors, matching of small problems, RANSAC bookkeeping, LM) that
    leave most of the chip's issue slots idle; a token (HIP event) passed from stream to stream serialises the
    median launches, so that while one part of the batch is in its median the other parts' latency-bound
    kernels fill the gaps.  Results are those of one FramePairPipeline over all B pairs, bit for bit (pair i
    samples with seed + i)."""

    class _Part(object):
        pass

    def __init__(self, device, gums, omni_shape, rig, n_pairs, n_streams=2, num_of_features=1000, kp_cap=512,
                 frame_cap=2048, max_iter=2000, adaptive=False, seed=0, detection_method="GFT", lm_iter=30, thr=None,
                 serialize_medians=True, ransac_solver="P3P", median_win_size=11, cross_check_stereo=False,
                 cross_check_f2f=False, gated_stereo=False, gated_f2f=False, gated_max_distance=None, ratio_stereo=False,
                 ratio_f2f=False, ratio=None, subpix=None, f2f_tracker="match", lk=None, stereo_refine=None, stereo_lk=None,
                 cyclic_columns=False):
        """median_win_size: StereoPanoramicFrame.median_win_size (11, pose_est_tools.py:296); 0 = no median blur (the
        RGB-D frames' setting, :427) -- then the colour panoramas are materialised and only converted to gray.
        cross_check_stereo ... cyclic_columns: as FramePairPipeline, in every part; a frame-to-frame matcher option with
        f2f_tracker="lk" raises ValueError."""
        from .frontend import DeviceImageModel, ImageFrontEnd
        from .parallel import shard_range
        so = StepOptions.of(cross_check_stereo, cross_check_f2f, gated_stereo, gated_f2f, gated_max_distance, ratio_stereo,
                            ratio_f2f, ratio, subpix, f2f_tracker, lk, stereo_refine, stereo_lk, cyclic_columns, rig,
                            detection_method=detection_method)
        self.lk, self.stereo_lk, self.cyclic = so.lk, so.stereo_lk, so.cyclic      # (checked before the device is touched)
        self.main = Context(device)                       # model constants + result collection: torch's current stream
        self.device = self.main.device
        self.model = DeviceImageModel(self.main, gums, omni_shape)
        m = self.model
        m.unwrap_table = self.main.unwrap_prepare(m.omni_masks, m.map_x, m.map_y, (m.H, m.W))
        if so.seam_free:    # the parts' front ends run on the padded panoramas
            m = m.seam_free_form(self.main)
        self.B, self.S = int(n_pairs), max(1, min(int(n_streams), int(n_pairs)))
        self.out = torch.zeros((self.B, 16), dtype=torch.float64, device=self.device)
        self.main.synchronize()
        self.parts = []
        for s in range(self.S):
            lo, hi = shard_range(self.B, s, self.S)
            p = self._Part()
            p.lo, p.hi = lo, hi
            p.stream = torch.cuda.Stream(self.device)
            with torch.cuda.stream(p.stream):
                p.ctx = Context(self.device.index, p.stream)
                if self.S > 1:
                    p.ctx.set_hint_shared_device(True)   # the parts run side by side: leave wave slots for each other
                p.fe = ImageFrontEnd(p.ctx, m, 2 * (hi - lo), detection_method=detection_method,
                                     num_of_features=num_of_features, kp_cap=kp_cap, keep_panoramas=False,
                                     median_win_size=median_win_size, subpix=subpix)
                p.pipe = FramePairPipeline(p.ctx, rig, hi - lo, frame_cap=frame_cap, max_iter=max_iter, adaptive=adaptive,
                                           seed=seed + lo, front_end=p.fe, lm_iter=lm_iter, thr=thr,
                                           ransac_solver=ransac_solver, **so.kwargs())
            p.median_done = torch.cuda.Event()
            p.done = torch.cuda.Event()
            self.parts.append(p)
        self.thr = self.parts[0].pipe.thr
        self.use_token = bool(serialize_medians)
        self._token = None       # the last median launch
        self._consumed = None    # self.out has been read by its consumer (see results())
        torch.cuda.synchronize(self.device)

    def contexts(self):
        return [p.ctx for p in self.parts]

    def load_frames(self, omni):
        """omni [2B,H,W,3] u8 (numpy or torch): pair i = frames 2i (reference) and 2i+1 (current)."""
        for p in self.parts:
            with torch.cuda.stream(p.stream):
                p.fe.load_frames(omni[2 * p.lo:2 * p.hi])
        torch.cuda.synchronize(self.device)

    def step_from_host(self, omni_pinned):
        """One pass over all B pairs whose omni frames are handed over in (pinned) HOST memory [2B,H,W,3] u8: every part
        copies its frames on the engine's copy stream into one of two device buffers (the copy for step k+1 overlaps the
        kernels of step k; a buffer is reused once the median that read it has finished) and then runs step()'s
        sequence.  This is the PCIe-inclusive form of the hot path."""
        k = self._host_step = getattr(self, "_host_step", -1) + 1
        j = k & 1
        if not hasattr(self, "_copy_streams"):
            # TWO copy streams shared by all parts (part i copies on stream i % 2): measured host-to-device rates with
            # three parts -- one queue 46 GB/s, two 55 GB/s, three 35 GB/s
            self._copy_streams = [torch.cuda.Stream(self.device) for _ in range(min(2, self.S))]
        for i, p in enumerate(self.parts):
            cs = self._copy_streams[i % len(self._copy_streams)]
            if not hasattr(p, "omni_bufs"):
                p.omni_bufs = [p.fe.omni, torch.empty_like(p.fe.omni)]
                p.copied = [torch.cuda.Event(), torch.cuda.Event()]
                # buffer 0 is the resident one: a preceding step()'s median on p.stream may still be reading it
                busy = torch.cuda.Event()
                busy.record(p.stream)
                p.omni_free = [busy, None]
            with torch.cuda.stream(cs):
                if p.omni_free[j] is not None:
                    cs.wait_event(p.omni_free[j])
                p.omni_bufs[j].copy_(omni_pinned[2 * p.lo:2 * p.hi], non_blocking=True)
                p.copied[j].record(cs)
            p.fe.omni = p.omni_bufs[j]
            p.stream.wait_event(p.copied[j])
        self.step(_after_median=lambda p: self._mark_free(p, j))

    @staticmethod
    def _mark_free(p, j):
        ev = torch.cuda.Event()
        ev.record(p.stream)
        p.omni_free[j] = ev

    def step(self, _after_median=None):
        """One pass of the whole hot path over all B pairs (asynchronous)."""
        for p in self.parts:
            with torch.cuda.stream(p.stream):
                if self._token is not None and self.use_token:
                    p.stream.wait_event(self._token)      # medians take turns
                p.fe.run_images()
                p.median_done.record(p.stream)
                self._token = p.median_done
                if _after_median is not None:
                    _after_median(p)
                p.fe.run_features()
                p.pipe.stereo()
                p.pipe.track()
                if self._consumed is not None:
                    p.stream.wait_event(self._consumed)   # the previous step's records have been read
                p.pipe.results(out=self.out[p.lo:p.hi])
                p.done.record(p.stream)

    def capture_graph(self):
        """One step() + results() of ALL parts captured into a torch.cuda.CUDAGraph; replay() then re-runs the whole
        hot path on the frames resident in the parts' buffers and leaves the records in self.out.
        What a correct capture needs: the parts' streams must JOIN the capture -- each waits on
        an event recorded on the capturing stream -- otherwise their kernels run eagerly, outside the graph, and a replay
        returns whatever the buffers hold; no wait may refer to an event recorded before the capture (the median token
        and the "records consumed" event of an earlier eager step); the per-kernel profile must be off (its event pairs
        would be captured and re-recorded); the library's scratch must have its final size (one eager step first)."""
        torch.cuda.synchronize(self.device)
        self.profile_enable(False)
        self._token, self._consumed = None, None
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            cur = torch.cuda.current_stream(self.device)
            fork = torch.cuda.Event()
            fork.record(cur)
            for p in self.parts:
                p.stream.wait_event(fork)
            self.step()
            self.results()          # the capturing stream waits for every part: the join
        self._token, self._consumed = None, None   # events recorded while capturing are nodes of the graph, not events
        torch.cuda.synchronize(self.device)
        return g

    def results(self):
        """[B,16] f64 records of the last step, valid on torch's current stream (which is made to wait for every
        part).  Call consumed() after enqueuing whatever reads them, before the next step()."""
        cur = torch.cuda.current_stream(self.device)
        for p in self.parts:
            cur.wait_event(p.done)
        return self.out

    def consumed(self):
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._consumed = ev

    def profile_enable(self, on=True):
        for p in self.parts:
            p.ctx.profile_enable(on)

    def profile_read(self):
        out = []
        for p in self.parts:
            out.extend(p.ctx.profile_read())
        return out

    def close(self):
        torch.cuda.synchronize(self.device)
        for p in self.parts:
            p.ctx.close()
        self.main.close()


def _batch_cfg(so, model, n_pairs, num_of_features, kp_cap, frame_cap, median_win_size, quality, min_distance, edge, thr, max_iter,
               adaptive, seed, lm_iter, ransac_solver, detection_method):
    """The `sosvo_batch_cfg` of FramePairBatch and SequenceEngine (n_pairs: pairs per call / slot pairs per tracking call) for
    the StepOptions `so` (its flags(); the settings of so.lk / so.stereo_lk belong to the context, see use_lk_options).
    kp_cap None = the detector's default capacity (frontend.default_kp_cap); thr None = the trackers' 5-degree threshold;
    any ransac_solver but "GP3P" is P3P."""
    from . import _lib, orb_pattern
    from .frontend import default_kp_cap
    detector = _lib.detector_code(detection_method)
    if kp_cap is None:
        kp_cap = default_kp_cap(str(detection_method).upper(), num_of_features)
    cos_a, sin_a = orb_pattern.angle_cos_sin(orb_pattern.GFT_KEYPOINT_ANGLE)
    c = _lib.BatchCfg()
    c.n_pairs, c.H, c.W, c.rows, c.cols, c.nmask = int(n_pairs), model.H, model.W, model.rows, model.cols, model.nmask
    c.kp_cap, c.frame_cap, c.median_ksize, c.max_corners, c.edge = int(kp_cap), int(frame_cap), int(median_win_size), \
        int(num_of_features), int(edge)
    c.ransac_max_iter, c.ransac_adaptive, c.lm_max_iter = int(max_iter), 1 if adaptive else 0, int(lm_iter)
    c.quality, c.min_distance = float(quality), float(min_distance)
    c.ransac_threshold = float(1.0 - np.cos(np.deg2rad(5.0))) if thr is None else float(thr)
    c.seed, c.cos_a, c.sin_a = int(seed), float(cos_a), float(sin_a)
    c.ransac_flags, c.detector = (_lib.FLAG_GP3P if str(ransac_solver).upper() == "GP3P" else 0) | so.flags(), detector
    return c


def batch_cfg(model, n_pairs, num_of_features, kp_cap, frame_cap, median_win_size, quality, min_distance, edge, thr, max_iter,
              adaptive, seed, lm_iter, ransac_solver, detection_method, cross_check_stereo=False, cross_check_f2f=False,
              gated_stereo=False, gated_f2f=False, gated_max_distance=None, ratio_stereo=False, ratio_f2f=False, ratio=None,
              subpix=None, lk=None, stereo_lk=None, cyclic_columns=False):
    """_batch_cfg with the options by name.  lk / stereo_lk: None, or the LKOptions / StereoLKOptions of an engine that tracks /
    refines its static stereo; what options go together is the caller's to check (StepOptions.of)."""
    detector_code(detection_method)      # (refused before a bad option, as ever)
    so = StepOptions.of(cross_check_stereo, cross_check_f2f, gated_stereo, gated_f2f, gated_max_distance, ratio_stereo, ratio_f2f,
                        ratio, subpix, order=("match", "subpix"))._replace(lk=lk, stereo_lk=stereo_lk, cyclic=cyclic_value(cyclic_columns))
    return _batch_cfg(so, model, n_pairs, num_of_features, kp_cap, frame_cap, median_win_size, quality, min_distance, edge, thr,
                      max_iter, adaptive, seed, lm_iter, ransac_solver, detection_method)


def _model_consts(ctx, model, so):
    """The model tensors a batched engine with the options `so` hands its front end when they are not the plain ones (None):
    the seam-free front end (SOSVO_FLAG_SEAM_FREE) takes the padded table and mask bits of the model's seam-free form."""
    if not so.seam_free:
        return None
    sf = model.seam_free_form(ctx)
    return sf.unwrap_table_run, sf.mask_bits_run, model.pattern


def use_lk_options(ctx, so):
    """Before a call of an engine with the StepOptions `so` that tracks (so.lk; None: it matches, nothing to do) or refines its
    static stereo (so.stereo_lk; None: it does not): contexts are shared between engines, so the context gets the settings
    whenever they differ from what it was last given."""
    if so.lk is not None and getattr(ctx, "lk_options", None) != so.lk:
        ctx.set_lk_options(so.lk)
    if so.stereo_lk is not None and getattr(ctx, "stereo_lk_options", None) != so.stereo_lk:
        ctx.set_stereo_lk_options(so.stereo_lk)


class FramePairBatch(object):
    """The same hot path behind ONE C-ABI call per step (sosvo_frame_pair_batch): what a non-Python host would
    bind.  `model` is a DeviceImageModel (model constants in HBM); the workspace is allocated once."""

    def __init__(self, ctx, model, rig, n_pairs, num_of_features=1000, kp_cap=None, frame_cap=2048, median_win_size=11,
                 quality=0.01, min_distance=5.0, edge=31, thr=None, max_iter=2000, adaptive=False, seed=0, lm_iter=30,
                 n_streams=1, ransac_solver="P3P", detection_method="GFT", cross_check_stereo=False, cross_check_f2f=False,
                 gated_stereo=False, gated_f2f=False, gated_max_distance=None, ratio_stereo=False, ratio_f2f=False, ratio=None,
                 subpix=None, f2f_tracker="match", lk=None, stereo_refine=None, stereo_lk=None, cyclic_columns=False):
        """n_streams > 1: sosvo_frame_pair_batch_streams (the batch split over internal HIP streams of the library).
        detection_method: "GFT", "ORB", "FAST" or "AGAST" -- the stages ImageFrontEnd runs for it; kp_cap None = its
        default capacity (frontend.default_kp_cap).
        cross_check_stereo ... cyclic_columns: as FramePairPipeline (the SOSVO_FLAG_* bits of cfg.ransac_flags), but subpix
        None = off, and a frame-to-frame matcher option with f2f_tracker="lk" raises ValueError."""
        so = StepOptions.of(cross_check_stereo, cross_check_f2f, gated_stereo, gated_f2f, gated_max_distance, ratio_stereo,
                            ratio_f2f, ratio, subpix, f2f_tracker, lk, stereo_refine, stereo_lk, cyclic_columns, rig,
                            store_levels=LK_MAX_LEVELS, detection_method=detection_method, edge=edge)
        self.options, self.lk, self.stereo_lk, self.cyclic = so, so.lk, so.stereo_lk, so.cyclic
        self.ctx, self.model, self.rig_cfg, self.rig = ctx, model, rig, rig.as_struct()
        self.B, self.n_streams = int(n_pairs), max(1, min(int(n_streams), int(n_pairs)))
        self.cfg = c = _batch_cfg(so, model, self.B, num_of_features=num_of_features, kp_cap=kp_cap, frame_cap=frame_cap,
                                  median_win_size=median_win_size, quality=quality, min_distance=min_distance, edge=edge, thr=thr,
                                  max_iter=max_iter, adaptive=adaptive, seed=seed, lm_iter=lm_iter, ransac_solver=ransac_solver,
                                  detection_method=detection_method)
        self.method = str(detection_method).upper()
        if getattr(model, "unwrap_table", None) is None:  # once per model
            model.unwrap_table = ctx.unwrap_prepare(model.omni_masks, model.map_x, model.map_y, (model.H, model.W))
        self._consts = _model_consts(ctx, model, so)
        nbytes = ctx.frame_pair_batch_workspace(c) if self.n_streams == 1 else ctx.frame_pair_batch_streams_workspace(c, self.n_streams)
        if nbytes <= 0:
            raise ValueError("bad batch configuration")
        self.workspace = torch.empty((nbytes,), dtype=torch.uint8, device=ctx.device)
        self.omni = torch.zeros((2 * self.B, model.H, model.W, 3), dtype=torch.uint8, device=ctx.device)
        self.out = torch.zeros((self.B, 16), dtype=torch.float64, device=ctx.device)

    def load_frames(self, omni):
        t = torch.from_numpy(np.ascontiguousarray(omni)) if isinstance(omni, np.ndarray) else omni
        self.omni.copy_(t.to(self.ctx.device))

    def step(self):
        """-> results [B,16] f64 (asynchronous)."""
        m = self.model
        use_lk_options(self.ctx, self.options)
        if self._consts is not None:
            return self.ctx.frame_pair_batch(self.rig, self.cfg, self.omni, *self._consts, self.workspace, results=self.out,
                                             n_streams=self.n_streams)
        return self.ctx.frame_pair_batch(self.rig, self.cfg, self.omni, m.unwrap_table, m.mask_bits, m.pattern, self.workspace,
                                         results=self.out, n_streams=self.n_streams)

    def enqueue(self, results=None):
        """A step WITHOUT the join (sosvo_frame_pair_batch_streams_enqueue, n_streams > 1): consecutive calls overlap on
        the library's internal streams.  Pass alternating `results` buffers while something still reads the previous
        step's records; call join() before reading records on the context's stream."""
        m = self.model
        use_lk_options(self.ctx, self.options)
        table, bits, pattern = self._consts or (m.unwrap_table, m.mask_bits, m.pattern)
        return self.ctx.frame_pair_batch(self.rig, self.cfg, self.omni, table, bits, pattern, self.workspace,
                                         results=self.out if results is None else results, n_streams=self.n_streams,
                                         join=self.n_streams <= 1)

    def join(self):
        if self.n_streams > 1:
            self.ctx.frame_pair_batch_join()

    def results(self):
        return self.out


_STAGE_POOL = None
_STAGE_POOL_LOCK = threading.Lock()   # (the lanes of a MultiSequenceEngine stage from several threads at once)
_STAGE_THREADS = 4


def _stage_rows(dst_np, images):
    """Frames of a window into a pinned staging buffer, four numpy copies at a time (numpy releases the GIL inside a large
    copy: 11.6 GB/s against 6.2 for one thread on the build container's cores -- a window of RGB-D frames is 69 MB.  torch's
    multi-threaded copy_ into PINNED memory, 26 GB/s here on pageable memory, ran at 0.5 GB/s on the GPU box)."""
    global _STAGE_POOL
    if len(images) < 4:
        for i, im in enumerate(images):
            np.copyto(dst_np[i], im)
        return
    with _STAGE_POOL_LOCK:
        if _STAGE_POOL is None:
            from concurrent.futures import ThreadPoolExecutor
            _STAGE_POOL = ThreadPoolExecutor(_STAGE_THREADS, thread_name_prefix="sosvo-stage")
    list(_STAGE_POOL.map(lambda i: np.copyto(dst_np[i], images[i]), range(len(images))))


class _SequenceFamily(object):
    """What the sequence engines of one family (omnistereo / RGB-D) keep for one frame store, and their device calls: `cfg`,
    the model constants, the workspace of `slots` slots, two pinned and two device input buffers of `frames` frames (a frame
    is a row of every tensor of a buffer: one tensor for omni images, two for (bgr, depth)) and, on request, the buffer a
    ragged round of a multi-sequence engine is gathered into.  `window` of the calls is `frames`.  A subclass sets up cfg
    and the constants and names its calls: `prefix` of the Context methods, `heads` (what the front-end calls take before
    cfg) and `track_heads` (the tracking calls), `consts()` (the model tensors of a front-end call), `shared` (the
    attributes an engine shows as its own)."""

    def _allocate(self, ctx, frames, slots, gather, frame_shapes):
        self.ctx, self.frames, self.slots = ctx, int(frames), int(slots)
        nbytes = self._call("workspace", ())
        if nbytes <= 0:   # (gather: the store of a multi-sequence engine)
            raise ValueError("bad sequence configuration" + (
                " (lanes * window: at most 8192 frames, lanes * (2 window + 1) <= 65535)" if gather else ""))
        dev = ctx.device
        self.workspace = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        new = lambda **kw: tuple(torch.zeros((self.frames,) + shape, dtype=dt, **kw) for shape, dt in frame_shapes)  # noqa: E731
        self._dev = [new(device=dev) for _ in range(2)]
        self._round = new(device=dev) if gather else None
        self._host = [tuple(t.pin_memory() for t in new()) for _ in range(2)]
        self._host_np = [tuple(t.numpy() for t in h) for h in self._host]

    def stage(self, buf, row, images):
        """images -> rows row .. of pinned buffer `buf`."""
        for dst, plane in zip(self._host_np[buf], self._planes(images)):
            _stage_rows(dst[row:row + len(plane)], plane)

    def upload(self, buf, row, n):
        for d, h in zip(self._dev[buf], self._host[buf]):
            d[row:row + n].copy_(h[row:row + n], non_blocking=True)

    def gather(self, buf, row, n, pos):
        for g, d in zip(self._round, self._dev[buf]):
            g[pos:pos + n].copy_(d[row:row + n], non_blocking=True)

    def rows(self, buf, row, n):
        """n frames of device buffer `buf` from `row` on (buf None: of the gathered round), as the front-end calls take them."""
        return tuple(t[row:row + n] for t in (self._round if buf is None else self._dev[buf]))

    def _call(self, name, heads, *args):
        return getattr(self.ctx, self.prefix + name)(*heads, self.cfg, self.frames, self.slots, *args)

    def front_end(self, rows, first_slot):
        self._call("front_end", self.heads, *rows, first_slot, *self.consts(), self.workspace)

    def front_end_slots(self, rows, table):
        self._call("front_end_slots", self.heads, *rows, table, *self.consts(), self.workspace)

    def track(self, ref_slots, cur_slots, seed, out):
        self._call("track", self.track_heads, ref_slots, cur_slots, seed, self.workspace, out)

    def track_seeds(self, ref_slots, cur_slots, seeds, out):
        self._call("track_seeds", self.track_heads, ref_slots, cur_slots, seeds, self.workspace, out)

    def counts(self, first, n):
        return self._call("frame_counts", (), first, n, self.workspace)

    def copy(self, src, dst):
        self._call("copy_slot", (), src, dst, self.workspace)

    def copy_slots(self, src, dst):
        self._call("copy_slots", (), src, dst, self.workspace)


class _OmniFamily(_SequenceFamily):
    prefix, shared = "sequence_", ("ctx", "cfg", "method", "workspace", "model", "rig_cfg", "rig")

    def __init__(self, ctx, model, rig, frames, slots, gather, so, **settings):
        """so: the engine's StepOptions; settings: _batch_cfg's tracker settings (num_of_features ... detection_method) but the seed."""
        assert isinstance(ctx, Context)
        self.model, self.rig_cfg, self.rig = model, rig, rig.as_struct()
        self.heads = self.track_heads = (self.rig,)
        self.options, self.lk, self.stereo_lk, self.cyclic = so, so.lk, so.stereo_lk, so.cyclic
        self.cfg = _batch_cfg(so, model, frames, seed=0, **settings)
        self.method = str(settings["detection_method"]).upper()
        if str(settings["ransac_solver"]).upper() not in ("P3P", "GP3P"):
            raise ValueError("ransac_solver: P3P or GP3P")
        if getattr(model, "unwrap_table", None) is None:  # once per model
            model.unwrap_table = ctx.unwrap_prepare(model.omni_masks, model.map_x, model.map_y, (model.H, model.W))
        self._consts = _model_consts(ctx, model, so)
        self._allocate(ctx, frames, slots, gather, [((model.H, model.W, 3), torch.uint8)])

    def consts(self):
        m = self.model
        return self._consts or (m.unwrap_table, m.mask_bits, m.pattern)

    def _call(self, name, heads, *args):
        """Engines that share a context may track with different settings: every device call of a tracking family runs under
        its own (the front end builds, the copies move and the tracker reads the pyramid levels they name)."""
        use_lk_options(self.ctx, self.options)
        return super()._call(name, heads, *args)

    @staticmethod
    def _planes(images):
        return (images,)


class _RGBDFamily(_SequenceFamily):
    prefix, track_heads = "rgbd_sequence_", ()
    shared = ("ctx", "cfg", "method", "workspace", "cam_cfg", "cam", "mask_bits", "pattern")

    def __init__(self, ctx, cam, frames, slots, gather, so, mask, **settings):
        """so: the engine's StepOptions; settings: _rgbd_batch_cfg's tracker settings (image_shape ... detection_method) but the seed."""
        from . import orb_pattern
        assert isinstance(ctx, Context)
        self.cam_cfg, self.cam = cam, cam.as_struct()
        self.heads = (self.cam,)
        self.cfg = c = _rgbd_batch_cfg(so, cam, frames, seed=0, **settings)
        self.method = str(settings["detection_method"]).upper()
        rows, cols = c.rows, c.cols
        mb = np.ones((1, rows, cols), np.uint32) if mask is None else (np.asarray(mask) != 0).astype(np.uint32).reshape(1, rows, cols)
        self.mask_bits = torch.from_numpy(mb).to(ctx.device)
        self.pattern = torch.from_numpy(orb_pattern.orb_pattern()).to(ctx.device)
        self._allocate(ctx, frames, slots, gather, [((rows, cols, 3), torch.uint8), ((rows, cols), torch.float32)])

    def consts(self):
        return self.mask_bits, self.pattern

    @staticmethod
    def _planes(images):   # (bgr, depth) tuples
        return [im[0] for im in images], [np.asarray(im[1], dtype=np.float32) for im in images]


def _adopt_family(engine, fam, **records):
    """The family's store is the engine's: what callers read on an engine (cfg, workspace, model constants, ...), and the
    engine's buffers of tracking records (name = rows)."""
    engine.fam = fam
    for name in fam.shared:
        setattr(engine, name, getattr(fam, name))
    for name, rows in records.items():
        setattr(engine, name, torch.zeros((rows, 16), dtype=torch.float64, device=fam.ctx.device))


class _SequenceBase(object):
    """Window / slot bookkeeping shared by the sequence engines (include/sosvo.h "Sequence mode"): two window halves
    [0, W) and [W, 2W) used alternately (the last frame of the previous window stays readable) and slot 2W for the current
    keyframe.  A tracking record is a pure function of (reference frame, current frame, seed): push_window() tracks every
    frame of the window against its PREDECESSOR in one batched call; the VO loop takes that record where the predecessor
    was the reference and asks for one serial track() call where it was not.  Either way the records are those of the
    serial loop, whatever the window size.  The hooks _stage_host / _upload / _front_end / _track / _counts / _copy go to the
    engine's family (self.fam, see _adopt).  The frames of a sequence are rows 0 .. of the family's buffers."""

    early_upload = True   # run_VO's staging thread starts a window's host-to-device copy itself (upload_staged); False: A/B
    enqueue_ahead = True  # run_VO enqueues window k + 1 before it works through window k's records (enqueue_staged); False: A/B
    _slot0 = 0            # first slot of this sequence's 2 W + 1 slots in the store (a lane of a MultiSequenceEngine: s (2 W + 1))

    def _init_windows(self, window):
        self.W = max(1, int(window))
        self.slots, self.key_slot = 2 * self.W + 1, self._slot0 + 2 * self.W
        self.reset()

    def _adopt(self, fam):
        _adopt_family(self, fam, spec=self.W, spec2=self.W, one=1)

    def _stage_host(self, images, buf):
        self.fam.stage(buf, 0, images)

    def _upload(self, buf, n):
        self.fam.upload(buf, 0, n)

    def _front_end(self, n, first, buf):
        self.fam.front_end(self.fam.rows(buf, 0, n), first)

    def _track(self, ref_slots, cur_slots, seed, out):
        self.fam.track(ref_slots, cur_slots, seed, out)

    def _counts(self, first, n):
        return self.fam.counts(first, n)

    def _copy(self, src, dst):
        self.fam.copy(src, dst)

    def reset(self):
        """Forget the sequence (an engine is reused from run to run: its buffers -- pinned host memory among them -- are the
        expensive part of its construction)."""
        self.half = 1            # the half the NEXT window goes to is 1 - half
        self.last_slot = None    # slot of the newest frame of the sequence
        self.last2_slot = None   # ... and of the one before it
        self.frames_seen = 0     # frames pushed so far (frame t of the sequence is tracked with seed t - 1)
        self.serial_calls = 0    # tracking calls the speculation did not cover
        self._key_src = None     # slot of a promoted frame whose record has not been copied to the keyframe slot yet
        if getattr(self, "_pending", None) is not None:
            self.ctx.synchronize()   # (a window an aborted run left on the stream: let it finish before its buffers are reused)
        self._pending = None     # the window enqueue_staged() put on the stream and collect() has not fetched yet
        self._up_pending = [0, 0]  # frames of pinned buffer b already on their way to device buffer b (upload_staged)
        if not hasattr(self, "_copy_stream"):
            self._copy_stream, self._up_event, self._win_events = None, None, None
        elif self._copy_stream is not None:
            self._copy_stream.synchronize()   # (a copy an aborted run left in flight)
        # host wall clock per stage; gpu_windows: the windows' own time on the stream (events around enqueue_staged's work)
        self.stage_s = dict(stage_to_pinned=0.0, enqueue=0.0, wait_and_readback=0.0, serial_track=0.0, gpu_windows=0.0)

    def push_window(self, images):
        """images: list of n <= window frames that continue the sequence (omnistereo: omni images [H,W,3] u8; RGB-D:
        (bgr, depth) tuples).  -> list of n dicts(slot, count = num_valid_keypoints, seed, spec_ref = slot the speculative
        record was tracked against or None, spec = that [16] record (numpy) or None).  One host synchronisation."""
        import time
        n = len(images)
        if n == 0:
            return []
        if n > self.W:
            raise ValueError("more frames than the window holds")
        t0 = time.perf_counter()
        self.stage_host(images, 0)
        self.stage_s["stage_to_pinned"] += time.perf_counter() - t0
        return self.push_staged(0, n)

    def stage_host(self, images, buf):
        """Copies the frames into pinned host buffer `buf` (0 / 1).  Touches nothing else: a helper thread may stage the NEXT
        window into the other buffer while this one is processed (numpy's copy releases the GIL) -- run_VO does."""
        self._stage_host(images, int(buf))

    def upload_staged(self, buf, n):
        """Starts the host-to-device copy of the n frames staged in pinned buffer `buf` on the engine's COPY stream, into
        device input buffer `buf`; push_staged(buf, n) then only waits for its event.  Optional: without it push_staged
        copies on the compute stream itself.  The helper thread that staged the window calls it (run_VO does), so the copy
        of window k + 1 runs on the DMA engines while window k's kernels run -- ~0.6 ms of 2.6 ms per window of 32 frames
        off the GPU-side critical path.  Buffer `buf` (host and device side) is free again when the push_staged that
        consumed it has returned (it synchronises)."""
        import torch
        buf, n = int(buf), int(n)
        if n <= 0:
            return
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=self.ctx.device)
            self._up_event = [torch.cuda.Event(), torch.cuda.Event()]
        with torch.cuda.stream(self._copy_stream):
            self._upload(buf, n)
            self._up_event[buf].record(self._copy_stream)
        self._up_pending[buf] = n

    def push_staged(self, buf, n):
        """push_window for n frames already staged in pinned buffer `buf`: enqueue_staged + collect."""
        if n == 0:
            return []
        self.enqueue_staged(buf, n)
        return self.collect()

    def enqueue_staged(self, buf, n):
        """The device work of push_staged(buf, n) WITHOUT waiting for it: copy (or the wait for upload_staged's copy), front end,
        the two speculative tracking batches.  collect() synchronises and returns the window's records.  A caller that has
        the next window ready enqueues it BEFORE it works through the records of the current one (run_VO does): the GPU
        then runs window k + 1 while the host's keyframe policy runs on window k.  What keeps that safe: the window halves
        alternate (window k + 1 refills the half of window k - 1), a promoted frame's record is copied to the keyframe slot
        before its half is refilled (here, as ever), serial track() calls read the keyframe slot and a slot of window k
        only, and everything is ordered on one stream.  One window may be pending."""
        import time
        self._check_push(n)
        t1 = time.perf_counter()
        buf = int(buf)
        if self._win_events is None:
            import torch
            self._win_events = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        w = self._plan_window(n)
        first = w["first"]
        if w["refills_promoted"]:
            self._flush_promotion()   # the promoted frame's record is about to be overwritten
        self._win_events[0].record(self.ctx.stream)
        if self._up_pending[buf] == n:            # copied ahead by upload_staged: order the compute stream behind it
            self.ctx.stream.wait_event(self._up_event[buf])
        else:
            self._upload(buf, n)
        self._up_pending[buf] = 0
        self._front_end(n, first, buf)
        if w["cur"]:
            self._track(w["prev"], w["cur"], w["seed0"], self.spec)
        if w["cur2"]:
            self._track(w["prev2"], w["cur2"], w["seed2"], self.spec2)
        self._win_events[1].record(self.ctx.stream)
        self._commit_window(w)
        self.stage_s["enqueue"] += time.perf_counter() - t1

    def _check_push(self, n):
        if n <= 0 or n > self.W:
            raise ValueError("1 .. window frames per push")
        if self._pending is not None:
            raise RuntimeError("collect() the pending window first")

    def _plan_window(self, n):
        """The bookkeeping of the next window of n frames, nothing on the device: the half it goes to, its slots, the slot
        pairs and seeds of the two speculative tracking batches.  (Flips self.half; _commit_window() does the rest.)"""
        self.half = 1 - self.half
        first = self._slot0 + self.half * self.W
        refills_promoted = self._key_src is not None and first <= self._key_src < first + self.W
        # speculative tracking: frame i of the window against its predecessor (the first one against the previous
        # window's last frame; the very first frame of the sequence has nothing to track against)
        slots = [first + i for i in range(n)]
        prev = ([self.last_slot] if self.last_slot is not None else []) + slots[:-1]
        cur = slots if self.last_slot is not None else slots[1:]
        seed0 = self.frames_seen - 1 if self.last_slot is not None else 0   # frame t tracks with seed t - 1
        # second guess: frame t against frame t - 2 -- the reference whenever frame t - 1 was NOT promoted to keyframe (then
        # the keyframe usually is t - 2: a frame is passed over when it has moved too little, rarely twice in a row).  Same
        # seeds (t - 1), so these are the records the serial call would return; what neither guess covers stays serial.
        # (a frame of the previous window is still in the store unless its slot lies in the half being refilled: window 1)
        alive = lambda s_: s_ is not None and not (first <= s_ < first + self.W)  # noqa: E731
        older = ([self.last2_slot] if alive(self.last2_slot) and alive(self.last_slot) else []) + \
            ([self.last_slot] if alive(self.last_slot) else []) + slots                       # frames ... t0-2, t0-1, t0, ...
        k0 = len(older) - n                                     # position of the window's first frame in `older`
        cur2 = [slots[i] for i in range(n) if k0 + i - 2 >= 0]
        prev2 = [older[k0 + i - 2] for i in range(n) if k0 + i - 2 >= 0]
        return dict(first=first, n=n, slots=slots, prev=prev, cur=cur, seed0=seed0, prev2=prev2, cur2=cur2,
                    seed2=self.frames_seen + (n - len(cur2)) - 1, refills_promoted=refills_promoted)

    def _commit_window(self, w):
        """The window planned by _plan_window() is on its way: it is the pending one, its frames are part of the sequence."""
        n, slots = w["n"], w["slots"]
        self._pending = dict(first=w["first"], n=n, slots=slots, prev=w["prev"], n_cur=len(w["cur"]), n_cur2=len(w["cur2"]),
                             frames_seen=self.frames_seen, had_last=self.last_slot is not None)
        self.frames_seen += n
        self.last2_slot = slots[-2] if n >= 2 else self.last_slot
        self.last_slot = slots[-1]

    def collect(self):
        """Waits for the window enqueue_staged() put on the stream and returns its n dicts (see push_window)."""
        import time
        p = self._pending
        if p is None:
            raise RuntimeError("no window pending")
        t2 = time.perf_counter()
        counts = self._counts(p["first"], p["n"])   # synchronises
        spec = self.spec[:p["n_cur"]].cpu().numpy() if p["n_cur"] else np.zeros((0, 16))
        spec2 = self.spec2[:p["n_cur2"]].cpu().numpy() if p["n_cur2"] else np.zeros((0, 16))
        self._pending = None
        self.stage_s["wait_and_readback"] += time.perf_counter() - t2
        self.stage_s["gpu_windows"] += 1e-3 * self._win_events[0].elapsed_time(self._win_events[1])
        return self._window_records(p, counts, spec, spec2)

    @staticmethod
    def _window_records(p, counts, spec, spec2):
        """The n dicts of a window (see push_window) from its plan, its slots' counts and its two speculative batches."""
        n, slots, prev = p["n"], p["slots"], p["prev"]
        out = []
        for i in range(n):
            t = p["frames_seen"] + i            # index of the frame in the sequence
            j = i if p["had_last"] else i - 1
            has = j >= 0 and p["n_cur"] > 0
            j2 = i - (n - p["n_cur2"])
            out.append(dict(slot=slots[i], count=counts[i], seed=max(t - 1, 0), spec_ref=prev[j] if has else None,
                            spec=spec[j].copy() if has else None, spec2=spec2[j2].copy() if j2 >= 0 else None))
        return out

    def track(self, ref_slot, cur_slot, seed):
        """One serial tracking call (reference slot, current slot, seed) -> [16] record (numpy); synchronises."""
        import time
        t0 = time.perf_counter()
        self.serial_calls += 1
        if int(ref_slot) == self.key_slot:
            self._flush_promotion()
        self._track([int(ref_slot)], [int(cur_slot)], int(seed), self.one)
        rec = self.one.cpu().numpy()[0]
        self.stage_s["serial_track"] += time.perf_counter() - t0
        return rec

    def promote(self, slot):
        """The frame in `slot` becomes the keyframe.  Its record moves to the keyframe slot LAZILY: when a serial tracking call
        reads that slot, or when the window half the frame lives in is about to be refilled -- most keyframes are replaced
        by the next one before either happens (242 of 256 frames of the bench sequence are promoted, 14 copies are made)."""
        self._key_src = int(slot)

    def _flush_promotion(self):
        if self._key_src is not None:
            self._copy(self._key_src, self.key_slot)
            self._key_src = None


class SequenceEngine(_SequenceBase):
    """Sequence mode of the SOS hot path (the reference's VO loop, run_VO, pose_est_tools.py:1416-1628): the front end of
    every frame is computed ONCE, `window` frames per batch, into a frame store in HBM, and frames are tracked against
    keyframes by slot number (see _SequenceBase)."""

    def __init__(self, ctx, model, rig, window=32, num_of_features=1000, kp_cap=None, frame_cap=2048, median_win_size=11,
                 quality=0.01, min_distance=5.0, edge=31, thr=None, max_iter=210, adaptive=True, lm_iter=30,
                 ransac_solver="GP3P", detection_method="GFT", cross_check_stereo=False, cross_check_f2f=False,
                 gated_stereo=False, gated_f2f=False, gated_max_distance=None, ratio_stereo=False, ratio_f2f=False, ratio=None,
                 subpix=None, f2f_tracker="match", lk=None, stereo_refine=None, stereo_lk=None, cyclic_columns=False):
        """Defaults: the trackers' settings (pose_est_tools.py:672-707: 5-degree threshold, the iteration budget of
        compute_num_of_iterations_RANSAC = 210 with the adaptive stop, generalised P3P; LM 30 iterations).
        detection_method and cross_check_stereo ... cyclic_columns: as FramePairBatch; with f2f_tracker="lk" the store keeps
        every frame's gray panoramas and their pyramid."""
        so = StepOptions.of(cross_check_stereo, cross_check_f2f, gated_stereo, gated_f2f, gated_max_distance, ratio_stereo,
                            ratio_f2f, ratio, subpix, f2f_tracker, lk, stereo_refine, stereo_lk, cyclic_columns, rig,
                            store_levels=LK_MAX_LEVELS, detection_method=detection_method, edge=edge)
        self._init_windows(window)
        self._adopt(_OmniFamily(ctx, model, rig, self.W, self.slots, False, so, num_of_features=num_of_features, kp_cap=kp_cap,
                                frame_cap=frame_cap, median_win_size=median_win_size, quality=quality, min_distance=min_distance,
                                edge=edge, thr=thr, max_iter=max_iter, adaptive=adaptive, lm_iter=lm_iter,
                                ransac_solver=ransac_solver, detection_method=detection_method))


def rgbd_solver_flags(pose_est_algorithm):
    """TrackerSE3.pose_est_algorithm (pose_est_tools.py:697; the names pyopengv.absolute_pose_ransac accepts, :89-107)
    -> the SOSVO_FLAG_* bits of the central RANSAC.  Unknown names raise, so that a batched engine can never silently run
    a different solver from the mirror tracker."""
    from . import _lib
    name = str(pose_est_algorithm).upper()
    table = {"EPNP": _lib.FLAG_EPNP, "KNEIP": 0, "GAO": _lib.FLAG_GP3P, "GP3P": _lib.FLAG_GP3P, "TWOPT": _lib.FLAG_TWOPT}
    if name not in table:
        raise ValueError("unknown pose_est_algorithm %r (have: %s)" % (pose_est_algorithm, ", ".join(sorted(table))))
    return table[name]


class RGBDCamConfig(object):
    """What the RGB-D hot path needs to know about the camera (host numbers): RGBDCamModel
    (omnistereo/camera_models.py:756-779), the RGBDFrame ranges (pose_est_tools.py:428-430, depth units) and
    TrackerRGBDSE3.bootstrap_tracker's |du| gate (pose_est_tools.py:956-958: 0.5 * 2 * center_x)."""

    def __init__(self, fx=525.0, fy=525.0, center_x=319.5, center_y=239.5, focal_length_m=1.0 / 1000.0, depth_is_Z=True,
                 min_range=0.8, max_range=7.0, f2f_max_hdiff=None, pct_good_matches=1.0):
        self.fx, self.fy, self.center_x, self.center_y = float(fx), float(fy), float(center_x), float(center_y)
        self.focal_length_m, self.depth_is_Z = float(focal_length_m), bool(depth_is_Z)
        self.min_range, self.max_range = float(min_range), float(max_range)
        self.f2f_max_hdiff = 0.5 * (2.0 * self.center_x) if f2f_max_hdiff is None else float(f2f_max_hdiff)
        self.pct_good_matches = float(pct_good_matches)

    def as_struct(self):
        from . import _lib
        c = _lib.RgbdCam()
        c.fx, c.fy, c.cx, c.cy, c.focal_length_m = self.fx, self.fy, self.center_x, self.center_y, self.focal_length_m
        c.depth_is_Z, c.reserved, c.min_range, c.max_range = 1 if self.depth_is_Z else 0, 0, self.min_range, self.max_range
        return c


def rgbd_kp_cap(method, num_of_features):
    """The RGB-D front ends' keypoint capacity per frame (RGBDFrontEnd, the engines, RGBDFrame): GFT > 1024 selects the
    detector's whole-image variant; ORB leaves retainBest head room (<= 2048, sosvo_detect_describe_orb); FAST / AGAST keep
    every corner up to the batch entry points' limit, 4096 (the first in raster order beyond it)."""
    method = str(method).upper()
    if method in ("FAST", "AGAST"):
        return 4096
    if method == "ORB":
        return int(min(2048, max(64, -(-int(num_of_features * 1.25) // 64) * 64)))
    return int(min(4096, max(1088, -(-int(num_of_features) // 64) * 64)))


class RGBDFrontEnd(object):
    """RGBDFrame.establish_keypoints (pose_est_tools.py:600-623) for F frames at once: [median,] gray,
    detection on the whole image (or RGBDFrame.mask) -- goodFeaturesToTrack, ORB, FAST or AGAST (:477-516) --, ORB
    descriptors, depth back-projection, NaN / range filter, bearings.  All buffers in HBM; four asynchronous C-ABI
    calls (three for ORB)."""

    def __init__(self, ctx, cam, nframes, image_shape=(480, 640), num_of_features=1000, kp_cap=None, frame_cap=None,
                 median_win_size=0, quality=0.01, min_distance=5.0, edge=31, mask=None, detection_method="GFT"):
        from . import _lib, orb_pattern
        assert isinstance(ctx, Context)
        _lib.detector_code(detection_method)   # (raises for the detectors that are not built)
        self.method = str(detection_method).upper()
        self.ctx, self.cam_cfg, self.cam = ctx, cam, cam.as_struct()
        self.F = int(nframes)
        self.rows, self.cols = int(image_shape[0]), int(image_shape[1])
        self.num_of_features, self.median_win_size = int(num_of_features), int(median_win_size)
        self.quality, self.min_distance, self.edge = float(quality), float(min_distance), int(edge)
        # GFT: > 1024 selects the detector's large-mask variant (whole-image masks), see sosvo_detect_gft
        self.kp_cap = int(kp_cap) if kp_cap else rgbd_kp_cap(self.method, self.num_of_features)
        self.frame_cap = int(frame_cap) if frame_cap else self.kp_cap
        dev, F = ctx.device, self.F
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        self.bgr = z((F, self.rows, self.cols, 3), torch.uint8)
        self.depth = z((F, self.rows, self.cols), torch.float32)
        self.gray = z((F, self.rows, self.cols), torch.uint8)
        mb = np.ones((1, self.rows, self.cols), np.uint32) if mask is None else \
            (np.asarray(mask) != 0).astype(np.uint32).reshape(1, self.rows, self.cols)
        self.mask_bits = torch.from_numpy(mb).to(dev)       # one mask (bit 0): RGBDFrame.mask or the whole image
        self.pattern = torch.from_numpy(orb_pattern.orb_pattern()).to(dev)
        self.cos_a, self.sin_a = orb_pattern.angle_cos_sin(orb_pattern.GFT_KEYPOINT_ANGLE)
        self.kp, self.n, self.status = DETECTED.alloc(dev, zeroed=True, P=F, cap=self.kp_cap).values()
        self.desc = ORB_DESC.alloc(dev, zeroed=True, P=F, cap=self.kp_cap)["desc"]
        if self.method == "ORB":
            self.kp4, self.resp = ORB.sub("kp4", "resp").alloc(dev, zeroed=True, P=F, cap=self.kp_cap).values()
            self.mask_pyr = ctx.orb_mask_pyramid(self.mask_bits, 1)   # once per mask
        self.frames = RGBD_FRAME.alloc(dev, zeroed=True, F=F, cap=self.frame_cap)

    def load_frames(self, bgr, depth):
        """bgr [F,rows,cols,3] u8, depth [F,rows,cols] f32 (the camera's depth units, 0 = no reading)."""
        dev = self.ctx.device
        self.bgr.copy_((torch.from_numpy(np.ascontiguousarray(bgr)) if isinstance(bgr, np.ndarray) else bgr).to(dev))
        self.depth.copy_((torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float32))
                          if isinstance(depth, np.ndarray) else depth).to(dev))

    def run(self):
        c = self.ctx
        c.median_gray(self.bgr, self.median_win_size, gray=self.gray)                              # :528, :531
        if self.method == "ORB":                                                                   # :478, :547, :553
            c.detect_describe_orb(self.gray, self.mask_pyr, self.F, 1, self.num_of_features, self.pattern, self.kp4,
                                  self.resp, self.n, self.desc, kp_xy=self.kp)
        else:
            if self.method in ("FAST", "AGAST"):                                                  # :506-509, :547
                (c.detect_fast if self.method == "FAST" else c.detect_agast)(
                    self.gray, self.mask_bits, self.F, 1, self.kp_cap, threshold=10, kp=self.kp, n=self.n,
                    status=self.status)
            else:
                c.detect_gft(self.gray, self.mask_bits, self.F, 1, self.kp_cap, quality=self.quality,
                             min_distance=self.min_distance, max_corners=self.num_of_features, kp=self.kp, n=self.n,
                             status=self.status)                                                    # :544
            c.describe_orb(self.gray, self.kp, self.n, 1, self.pattern, self.cos_a, self.sin_a, edge=self.edge,
                           desc=self.desc)                                                          # :553
        c.rgbd_assemble(self.cam, self.kp, self.desc, self.n, self.depth, self.frame_cap, out=self.frames)  # :609-623


class RGBDPairPipeline(object):
    """The RGB-D (perspective) counterpart of ImageFrontEnd + FramePairPipeline (BASELINE config 5): for B
    independent pairs of (BGR image, depth map) frames, RGBDFrontEnd and then TrackerRGBDSE3.track_frame
    (pose_est_tools.py:896-954: frame-to-frame matching, |du| gate, central RANSAC, LM).
    Pair i tracks frame 2i+1 against frame 2i.  Everything stays in HBM; one step = 10 asynchronous C-ABI calls."""

    def __init__(self, ctx, cam, n_pairs, image_shape=(480, 640), num_of_features=1000, kp_cap=None, frame_cap=None,
                 median_win_size=0, quality=0.01, min_distance=5.0, edge=31, thr=None, max_iter=2000, adaptive=False,
                 seed=0, lm_iter=30, mask=None, pose_est_algorithm="EPNP", detection_method="GFT", cross_check=False,
                 gated_f2f=False, gated_max_distance=None, ratio_f2f=False, ratio=None):
        """detection_method: "GFT", "ORB", "FAST" or "AGAST" (RGBDFrontEnd).
        cross_check, gated_f2f ... ratio: FramePairPipeline's cross_check_f2f, gated_f2f ... ratio, in the one matcher of an
        RGB-D camera (feature_matcher_for_motion; the gate is the tracker's |du| gate).
        pose_est_algorithm: TrackerSE3.pose_est_algorithm (pose_est_tools.py:697): "EPNP" = 6-point samples solved by
        EPnP; "KNEIP" = P3P on 3 points + a 4th for disambiguation; "GAO" / "GP3P" = the depth formulation through the
        generalised solver; "TWOPT" = translation from 2 points.  Anything else raises ValueError."""
        from . import _lib
        self.ctx, self.cam_cfg = ctx, cam
        self.solver_flags = rgbd_solver_flags(pose_est_algorithm)
        self.epnp = bool(self.solver_flags & _lib.FLAG_EPNP)
        self.B, self.F = int(n_pairs), 2 * int(n_pairs)
        fe = RGBDFrontEnd(ctx, cam, self.F, image_shape, num_of_features, kp_cap, frame_cap, median_win_size, quality,
                          min_distance, edge, mask, detection_method=detection_method)
        self.front_end, self.frames, self.kp_cap, self.frame_cap = fe, fe.frames, fe.kp_cap, fe.frame_cap
        self.n, self.status, self.kp, self.desc, self.gray = fe.n, fe.status, fe.kp, fe.desc, fe.gray
        self.thr = float(1.0 - np.cos(np.deg2rad(5.0))) if thr is None else float(thr)
        self.max_iter, self.adaptive, self.seed, self.lm_iter = int(max_iter), bool(adaptive), int(seed), int(lm_iter)
        dev, F, B, Fc = ctx.device, self.F, self.B, self.frame_cap
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        self.ref_frame = torch.arange(0, F, 2, dtype=torch.int32, device=dev)
        self.cur_frame = torch.arange(1, F, 2, dtype=torch.int32, device=dev)
        self.order = z((B, Fc), torch.int32)
        # (ValueError for a cap out of range, a ratio that is no 64th)
        self.opts = o = StepOptions.rgbd(cross_check, gated_f2f, gated_max_distance, ratio_f2f, ratio).match
        q, t = self.cur_frame, self.ref_frame
        if o.cross_check_f2f:   # the B role-swapped problems ride in the same launch, after the forward ones
            q, t = torch.cat([q, t]), torch.cat([t, q])
        self._q, self._t, self._k = q, t, z((len(q), Fc, 1), torch.uint32)
        self.cur_frame, self.ref_frame, self.keys = q[:B], t[:B], self._k[:B]     # the forward problems
        # what track() hands the matching step: the |du| gate of f2f_assemble_central
        self._f2f_search = dict(ratio_64ths=o.ratio_64ths_f2f, rivals=torch.zeros_like(self._k) if o.ratio_f2f else None,
                                gate=(-1.0, cam.f2f_max_hdiff, gated_max_distance) if o.gated_f2f else None)
        self.corr = CORR_CENTRAL.alloc(dev, zeroed=True, NP=B, cap=Fc)
        self.ransac = RANSAC.alloc(dev, zeroed=True, P=B, S=Fc)
        self.T = z((B, 3, 4), torch.float64)
        self.lm_cost, self.lm_iters = z((B,), torch.float64), z((B,), torch.int32)

    def load_frames(self, bgr, depth):
        self.front_end.load_frames(bgr, depth)

    def detect(self):
        self.front_end.run()

    def track(self):
        c, fr, cfg = self.ctx, self.frames, self.cam_cfg
        c.match_1nn_slots(fr["d"], fr["m"], fr["M"], self._q, self._t, self._k, self.B, **self._f2f_search)
        c.sort_matches(self.keys, fr["M"], order=self.order, q_slot=self.cur_frame)
        c.f2f_assemble_central(fr, self.ref_frame, self.cur_frame, self.keys, self.order, self.frame_cap,
                               pct_good_matches=cfg.pct_good_matches, max_hdiff=cfg.f2f_max_hdiff, out=self.corr)
        co = self.corr
        from . import _lib
        c.ransac_abs_pose(co["f"], co["p"], co["n"], self.thr, self.max_iter, seed=self.seed, adaptive=self.adaptive,
                          out=self.ransac, epnp=self.epnp, gp3p=bool(self.solver_flags & _lib.FLAG_GP3P),
                          twopt=bool(self.solver_flags & _lib.FLAG_TWOPT))                          # :915 (central)
        self.T.copy_(self.ransac["T"])
        c.refine_abs_pose(co["f"], co["p"], co["n"], self.T, idx=self.ransac["idx"], m=self.ransac["n_inliers"],
                          max_lm_iter=self.lm_iter, cost=self.lm_cost, iters=self.lm_iters)          # :937

    def step(self):
        self.detect()
        self.track()
        return self.T

    def results(self):
        """[B,16] f64 rows as FramePairPipeline.results()."""
        out = torch.empty((self.B, 16), dtype=torch.float64, device=self.ctx.device)
        out[:, :12] = self.T.reshape(self.B, 12)
        out[:, 12] = self.ransac["n_inliers"].to(torch.float64)
        out[:, 13] = self.corr["n"].to(torch.float64)
        out[:, 14] = self.ransac["info"][:, 2].to(torch.float64)
        out[:, 15] = self.ransac["info"][:, 0].to(torch.float64)
        return out


def _rgbd_batch_cfg(so, cam, n_pairs, image_shape, num_of_features, kp_cap, frame_cap, median_win_size, quality, min_distance, edge,
                    thr, max_iter, adaptive, seed, lm_iter, pose_est_algorithm, detection_method):
    """The `sosvo_rgbd_batch_cfg` of RGBDPairBatch and RGBDSequenceEngine (n_pairs: pairs per call / slot pairs per tracking
    call; cam: an RGBDCamConfig) for the StepOptions `so` (StepOptions.rgbd).  kp_cap None or 0 = rgbd_kp_cap; frame_cap None
    or 0 = kp_cap; thr None = the trackers' 5-degree threshold."""
    from . import _lib, orb_pattern
    detector_flags = _lib.rgbd_detector_flags(detection_method)
    kp_cap = int(kp_cap) if kp_cap else rgbd_kp_cap(str(detection_method).upper(), num_of_features)
    cos_a, sin_a = orb_pattern.angle_cos_sin(orb_pattern.GFT_KEYPOINT_ANGLE)
    c = _lib.RgbdBatchCfg()
    c.n_pairs, c.rows, c.cols = int(n_pairs), int(image_shape[0]), int(image_shape[1])
    c.kp_cap, c.frame_cap = kp_cap, int(frame_cap) if frame_cap else kp_cap
    c.median_ksize, c.max_corners, c.edge = int(median_win_size), int(num_of_features), int(edge)
    c.ransac_max_iter, c.ransac_adaptive, c.lm_max_iter = int(max_iter), 1 if adaptive else 0, int(lm_iter)
    c.flags = rgbd_solver_flags(pose_est_algorithm) | detector_flags | so.flags()
    c.quality, c.min_distance = float(quality), float(min_distance)
    c.ransac_threshold = float(1.0 - np.cos(np.deg2rad(5.0))) if thr is None else float(thr)
    c.pct_good_matches, c.f2f_max_hdiff = float(cam.pct_good_matches), float(cam.f2f_max_hdiff)
    c.seed, c.cos_a, c.sin_a = int(seed), float(cos_a), float(sin_a)
    return c


def rgbd_batch_cfg(cam, n_pairs, image_shape, num_of_features, kp_cap, frame_cap, median_win_size, quality, min_distance, edge,
                   thr, max_iter, adaptive, seed, lm_iter, pose_est_algorithm, detection_method, cross_check=False, gated_f2f=False,
                   gated_max_distance=None, ratio_f2f=False, ratio=None):
    """_rgbd_batch_cfg with the options by name."""
    rgbd_detector_flags(detection_method), rgbd_solver_flags(pose_est_algorithm)      # (refused before a bad option, as ever)
    return _rgbd_batch_cfg(StepOptions.rgbd(cross_check, gated_f2f, gated_max_distance, ratio_f2f, ratio), cam, n_pairs, image_shape,
                           num_of_features, kp_cap, frame_cap, median_win_size, quality, min_distance, edge, thr, max_iter, adaptive,
                           seed, lm_iter, pose_est_algorithm, detection_method)


class RGBDPairBatch(object):
    """RGBDPairPipeline behind ONE C-ABI call per step (sosvo_rgbd_pair_batch): what a non-Python host would bind for
    BASELINE config 5.  Same arguments and results as RGBDPairPipeline; the workspace is allocated once."""

    def __init__(self, ctx, cam, n_pairs, image_shape=(480, 640), num_of_features=1000, kp_cap=None, frame_cap=None,
                 median_win_size=0, quality=0.01, min_distance=5.0, edge=31, thr=None, max_iter=2000, adaptive=False,
                 seed=0, lm_iter=30, mask=None, pose_est_algorithm="EPNP", detection_method="GFT", cross_check=False,
                 gated_f2f=False, gated_max_distance=None, ratio_f2f=False, ratio=None, f2f_tracker="match", lk=None,
                 stereo_refine=None, stereo_lk=None, cyclic_columns=False):
        from . import orb_pattern
        so = StepOptions.rgbd(cross_check, gated_f2f, gated_max_distance, ratio_f2f, ratio, f2f_tracker, lk, stereo_refine, stereo_lk,
                              cyclic_columns)      # (a tracker, a stereo refinement, cyclic columns: ValueError)
        self.ctx, self.cam_cfg, self.cam = ctx, cam, cam.as_struct()
        self.B = int(n_pairs)
        c = _rgbd_batch_cfg(so, cam, self.B, seed=seed, image_shape=image_shape, num_of_features=num_of_features, kp_cap=kp_cap,
                            frame_cap=frame_cap, median_win_size=median_win_size, quality=quality, min_distance=min_distance,
                            edge=edge, thr=thr, max_iter=max_iter, adaptive=adaptive, lm_iter=lm_iter,
                            pose_est_algorithm=pose_est_algorithm, detection_method=detection_method)
        self.method = str(detection_method).upper()
        rows, cols = c.rows, c.cols
        self.cfg, self.thr = c, c.ransac_threshold
        dev = ctx.device
        mb = np.ones((1, rows, cols), np.uint32) if mask is None else (np.asarray(mask) != 0).astype(np.uint32).reshape(1, rows, cols)
        self.mask_bits = torch.from_numpy(mb).to(dev)
        self.pattern = torch.from_numpy(orb_pattern.orb_pattern()).to(dev)
        nbytes = ctx.rgbd_pair_batch_workspace(c)
        if nbytes <= 0:
            raise ValueError("bad batch configuration")
        self.workspace = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        self.bgr = torch.zeros((2 * self.B, rows, cols, 3), dtype=torch.uint8, device=dev)
        self.depth = torch.zeros((2 * self.B, rows, cols), dtype=torch.float32, device=dev)
        self.out = torch.zeros((self.B, 16), dtype=torch.float64, device=dev)

    def load_frames(self, bgr, depth):
        dev = self.ctx.device
        self.bgr.copy_((torch.from_numpy(np.ascontiguousarray(bgr)) if isinstance(bgr, np.ndarray) else bgr).to(dev))
        self.depth.copy_((torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float32))
                          if isinstance(depth, np.ndarray) else depth).to(dev))

    def step(self):
        """-> results [B,16] f64 (asynchronous)."""
        return self.ctx.rgbd_pair_batch(self.cam, self.cfg, self.bgr, self.depth, self.mask_bits, self.pattern, self.workspace,
                                        results=self.out)

    def results(self):
        return self.out


class RGBDSequenceEngine(_SequenceBase):
    """Sequence mode of the RGB-D path (demo_vo_rgbd.py's loop: one RGBDFrame per image, pose_est_tools.py:1440-1446, tracked
    against the current keyframe, :896-954) on the sosvo_rgbd_sequence_* entry points; push_window() takes (bgr, depth)
    tuples.  Same store layout, seeds and speculation as SequenceEngine."""

    def __init__(self, ctx, cam, window=32, image_shape=(480, 640), num_of_features=1000, kp_cap=None, frame_cap=None,
                 median_win_size=0, quality=0.01, min_distance=5.0, edge=31, thr=None, max_iter=210, adaptive=True, lm_iter=30,
                 mask=None, pose_est_algorithm="EPNP", detection_method="GFT", cross_check=False, gated_f2f=False,
                 gated_max_distance=None, ratio_f2f=False, ratio=None, f2f_tracker="match", lk=None, stereo_refine=None,
                 stereo_lk=None, cyclic_columns=False):
        so = StepOptions.rgbd(cross_check, gated_f2f, gated_max_distance, ratio_f2f, ratio, f2f_tracker, lk, stereo_refine, stereo_lk,
                              cyclic_columns)      # (a tracker, a stereo refinement, cyclic columns: ValueError)
        self._init_windows(window)
        self._adopt(_RGBDFamily(ctx, cam, self.W, self.slots, False, so, mask,
                                image_shape=image_shape, num_of_features=num_of_features, kp_cap=kp_cap,
                                frame_cap=frame_cap, median_win_size=median_win_size, quality=quality, min_distance=min_distance,
                                edge=edge, thr=thr, max_iter=max_iter, adaptive=adaptive, lm_iter=lm_iter,
                                pose_est_algorithm=pose_est_algorithm, detection_method=detection_method))


# ---- several sequences ("lanes") through one engine ----------------------------------------------------------------------
class _Lane(_SequenceBase):
    """One sequence of a multi-sequence engine: the bookkeeping of _SequenceBase over its own 2 W + 1 slots of the shared
    store, with the interface run_VO, sequence_windows, the device frames and the trackers use.  It makes no device call
    of its own: enqueue_staged(), track() and a promotion that has to be flushed file REQUESTS with the engine, collect()
    and track() park the calling thread until the engine has served them (see _MultiSequenceBase)."""

    def __init__(self, engine, index):
        self.engine, self.index, self.ctx = engine, int(index), engine.ctx
        self.cfg = engine.cfg
        for name in ("rig_cfg", "cam_cfg", "method", "model"):
            if hasattr(engine, name):
                setattr(self, name, getattr(engine, name))
        self._slot0 = self.index * (2 * engine.W + 1)
        self._win_req = self._win_res = self._track_req = self._track_res = self._copy_req = None
        self._init_windows(engine.W)

    def reset(self):
        eng = self.engine
        with eng._cv:
            # (a window that was served has been read back, one that was not never reached the stream: nothing of an aborted
            # run is left on the compute stream; an upload it started ahead may still read the lane's pinned rows)
            self._pending = None
            self._win_req = self._win_res = self._track_req = self._track_res = self._copy_req = None
            if eng._copy_stream is not None:
                eng._copy_stream.synchronize()
            self._up_ahead = [0, 0]      # frames of pinned buffer b already on their way to this lane's device rows b
            _SequenceBase.reset(self)

    def stage_host(self, images, buf):
        self.engine._stage_lane(self.index, images, int(buf))

    def upload_staged(self, buf, n):
        buf, n = int(buf), int(n)
        if n > 0:
            self.engine._upload_ahead(self, buf, n)

    def enqueue_staged(self, buf, n):
        """Files the window (n frames staged in pinned buffer `buf`) with the engine; nothing reaches the device before every
        live lane waits for the engine."""
        import time
        self._check_push(n)
        t1 = time.perf_counter()
        with self.engine._cv:
            w = self._plan_window(n)
            if w["refills_promoted"]:
                self._flush_promotion()
            w["buf"] = int(buf)
            self._win_req, self._win_res = w, None
            self._commit_window(w)
        self.stage_s["enqueue"] += time.perf_counter() - t1

    def collect(self):
        import time
        p = self._pending
        if p is None:
            raise RuntimeError("no window pending")
        t2 = time.perf_counter()
        self.engine._park(self, lambda: self._win_res is not None)
        res, self._win_res, self._pending = self._win_res, None, None
        self.stage_s["wait_and_readback"] += time.perf_counter() - t2
        self.stage_s["gpu_windows"] += res["gpu_s"]
        return self._window_records(p, res["counts"], res["spec"], res["spec2"])

    def track(self, ref_slot, cur_slot, seed):
        import time
        t0 = time.perf_counter()
        self.serial_calls += 1
        with self.engine._cv:
            if int(ref_slot) == self.key_slot:
                self._flush_promotion()
            self._track_req, self._track_res = (int(ref_slot), int(cur_slot), int(seed)), None
        self.engine._park(self, lambda: self._track_res is not None)
        rec, self._track_res = self._track_res, None
        self.stage_s["serial_track"] += time.perf_counter() - t0
        return rec

    def _flush_promotion(self):
        # (a later promotion of this lane replaces one that has not been served: both go to the lane's keyframe slot, and
        # nothing reads that slot in between -- a reader parks the lane, which gets the request served)
        if self._key_src is not None:
            self._copy_req = (self._key_src, self.key_slot)
            self._key_src = None


class _MultiSequenceBase(object):
    """S sequences ("lanes") that share one camera model through ONE frame store, one stream and one launch per stage and
    round (include/sosvo.h "Several sequences through one frame store").  lane(s) is an object with the interface of a
    single-sequence engine; each lane is driven by its own host thread (run_VO_many: one run_VO per lane).  The lanes'
    requests -- windows, serial tracking calls, promotions to flush -- are only FILED; when every live lane waits for the
    engine (collect() or track()), the thread that parked last serves everything pending, grouped by kind:
        promotions  -> one ..._copy_slots call
        windows     -> one ..._front_end_slots call over all their frames, one ..._track_seeds call for the first guesses
                       (t against t - 1), one for the second (t against t - 2)
        track()     -> one ..._track_seeds call
    and ONE read-back, then wakes the lanes.  A frame record is a function of its image, a tracking record of (reference
    record, current record, seed): which call computes a record never changes it, so the lanes' results are those of S
    single-sequence engines whatever the grouping.  begin(s) / end(s) bracket a lane's run (a lane that is not live is not
    waited for).  The hooks _stage_lane / _upload_lane / _gather_lane / _front_end_round / _track_seeds / _counts_all /
    _copy_slots go to the engine's family (self.fam, see _adopt); lane s owns rows s W .. of the family's buffers."""

    def _init_lanes(self, lanes, window):
        self.S, self.W = max(1, int(lanes)), max(1, int(window))
        self.window, self.slots = self.S * self.W, self.S * (2 * self.W + 1)
        self._cv = threading.Condition(threading.RLock())
        self._live, self._parked, self._error = set(), set(), None
        self._copy_stream = self._up_events = self._round_events = None
        self._up_lock = threading.Lock()
        self.reset_counters()

    def _make_lanes(self):
        self.lanes = [_Lane(self, s) for s in range(self.S)]

    def _adopt(self, fam):
        _adopt_family(self, fam, spec=self.window, spec2=self.window, serial=self.S)
        self._make_lanes()

    def _stage_lane(self, s, images, buf):
        self.fam.stage(buf, s * self.W, images)

    def _upload_lane(self, s, buf, n):
        self.fam.upload(buf, s * self.W, n)

    def _gather_lane(self, s, buf, n, pos):
        self.fam.gather(buf, s * self.W, n, pos)

    def _front_end_round(self, requests, slot_of_frame):
        buf, row, n = self._input_rows(requests)
        self.fam.front_end_slots(self.fam.rows(buf, row, n), slot_of_frame)

    def _track_seeds(self, ref_slots, cur_slots, seeds, out):
        self.fam.track_seeds(ref_slots, cur_slots, seeds, out)

    def _counts_all(self):
        return self.fam.counts(0, self.slots)

    def _copy_slots(self, src, dst):
        self.fam.copy_slots(src, dst)

    def reset_counters(self):
        """front_end_launches / speculative_track_launches / serial_track_launches / copy_launches: device calls made;
        max_serial_pairs: the largest number of pairs in one serial launch; rounds: serves that held a window;
        gpu_windows: the rounds' own time on the stream (events around the front end and the speculative batches), seconds."""
        self.counters = dict(front_end_launches=0, speculative_track_launches=0, serial_track_launches=0, max_serial_pairs=0,
                             copy_launches=0, rounds=0, host_syncs=0, gpu_windows=0.0)

    def lane(self, s):
        return self.lanes[int(s)]

    def begin(self, s):
        """Lane s starts a sequence: it is reset and the engine waits for it from now on."""
        lane = self.lanes[int(s)]
        lane.reset()
        with self._cv:
            self._live.add(lane.index)
        return lane

    def end(self, s):
        """Lane s has finished (sequence exhausted, failed, aborted): its unserved requests are dropped and the others no
        longer wait for it."""
        lane = self.lanes[int(s)]
        with self._cv:
            self._live.discard(lane.index)
            self._parked.discard(lane.index)
            lane._win_req = lane._track_req = lane._copy_req = None
            self._serve_if_due()
            self._cv.notify_all()

    def _park(self, lane, ready):
        with self._cv:
            if lane.index not in self._live:     # (a lane used on its own, without begin(): served at once)
                if not ready():
                    self._serve()
                return
            try:
                while not ready():
                    self._parked.add(lane.index)
                    if self._error is not None:
                        raise RuntimeError("a device call of the multi-sequence engine failed") from self._error
                    if self._live <= self._parked:
                        self._serve()
                        self._cv.notify_all()
                    else:
                        self._cv.wait()
            finally:
                self._parked.discard(lane.index)

    def _serve_if_due(self):
        if self._live and self._live <= self._parked and self._error is None:
            self._serve()

    def _serve(self):
        try:
            self._serve_requests()
            # every parked lane had a request, and it has been served: none of them waits any more, whenever its thread gets
            # to notice (a lane that files its next request before the others have woken up must not take them for parked)
            self._parked.clear()
        except BaseException as e:
            self._error = e
            self._cv.notify_all()
            raise

    def _serve_requests(self):
        """Everything filed, grouped by kind, on the stream; one read-back.  (Called with the lock held.)"""
        c = self.counters
        copies = [l for l in self.lanes if l._copy_req is not None]
        wins = [l for l in self.lanes if l._win_req is not None]
        tracks = [l for l in self.lanes if l._track_req is not None]
        if not (copies or wins or tracks):
            return
        with self._stream_scope():
            if copies:      # before anything refills a promoted frame's half or reads a keyframe slot
                self._copy_slots([l._copy_req[0] for l in copies], [l._copy_req[1] for l in copies])
                c["copy_launches"] += 1
                for l in copies:
                    l._copy_req = None
            n_spec = n_spec2 = 0
            if wins:
                if self._round_events is None:
                    self._round_events = self._timing_events()
                self._round_events[0].record(self.ctx.stream)
                self._front_end_round([(l.index, l._win_req["buf"], l._win_req["n"]) for l in wins],
                                      [s_ for l in wins for s_ in l._win_req["slots"]])
                c["front_end_launches"] += 1
                ref = [s_ for l in wins for s_ in l._win_req["prev"]]
                cur = [s_ for l in wins for s_ in l._win_req["cur"]]
                seeds = [l._win_req["seed0"] + i for l in wins for i in range(len(l._win_req["cur"]))]
                n_spec = len(cur)
                if n_spec:
                    self._track_seeds(ref, cur, seeds, self.spec)
                    c["speculative_track_launches"] += 1
                ref2 = [s_ for l in wins for s_ in l._win_req["prev2"]]
                cur2 = [s_ for l in wins for s_ in l._win_req["cur2"]]
                seeds2 = [l._win_req["seed2"] + i for l in wins for i in range(len(l._win_req["cur2"]))]
                n_spec2 = len(cur2)
                if n_spec2:
                    self._track_seeds(ref2, cur2, seeds2, self.spec2)
                    c["speculative_track_launches"] += 1
                self._round_events[1].record(self.ctx.stream)
            if tracks:
                self._track_seeds([l._track_req[0] for l in tracks], [l._track_req[1] for l in tracks],
                                  [l._track_req[2] for l in tracks], self.serial)
                c["serial_track_launches"] += 1
                c["max_serial_pairs"] = max(c["max_serial_pairs"], len(tracks))
            # ---- one read-back for the round
            c["host_syncs"] += 1
            if wins:
                counts = self._counts_all()      # synchronises
                spec = self.spec[:n_spec].cpu().numpy() if n_spec else np.zeros((0, 16))
                spec2 = self.spec2[:n_spec2].cpu().numpy() if n_spec2 else np.zeros((0, 16))
                gpu_s = 1e-3 * self._round_events[0].elapsed_time(self._round_events[1])
                c["rounds"] += 1
                c["gpu_windows"] += gpu_s
                frames = sum(l._win_req["n"] for l in wins)
                o1 = o2 = 0
                for l in wins:
                    w = l._win_req
                    n1, n2 = len(w["cur"]), len(w["cur2"])
                    l._win_res = dict(counts=[counts[s_] for s_ in w["slots"]], spec=spec[o1:o1 + n1], spec2=spec2[o2:o2 + n2],
                                      gpu_s=gpu_s * w["n"] / frames)     # (the round's time, shared out by frames)
                    l._win_req = None
                    o1, o2 = o1 + n1, o2 + n2
            if tracks:
                recs = self.serial[:len(tracks)].cpu().numpy()   # synchronises
                for i, l in enumerate(tracks):
                    l._track_res, l._track_req = recs[i].copy(), None

    def _stream_scope(self):
        """(the serving thread is any lane's: its torch work goes to the context's stream, whatever that thread's current one)"""
        return torch.cuda.stream(self.ctx.stream)

    @staticmethod
    def _timing_events():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    # (the lanes' early uploads: one copy stream, one event per (lane, buffer))
    def _upload_ahead(self, lane, buf, n):
        # Not under the engine's lock: a serve holds that across its read-back, and the copy of window k + 1 is meant to run
        # beside round k.  What it touches is the lane's own: rows (lane, buf) of the input buffers and their event are free
        # from the collect() of the window that used them until the enqueue_staged() of this one, which the staging thread
        # orders after this call (sequence_windows' ready queue).
        with self._up_lock:
            if self._copy_stream is None:
                self._up_events = [[torch.cuda.Event(), torch.cuda.Event()] for _ in range(self.S)]
                self._copy_stream = torch.cuda.Stream(device=self.ctx.device)
            stream = self._copy_stream
        with torch.cuda.stream(stream):
            self._upload_lane(lane.index, buf, n)
            self._up_events[lane.index][buf].record(stream)
        lane._up_ahead[buf] = n

    def _input_rows(self, requests):
        """requests: [(lane, buf, n)] of a round.  Every lane's frames are brought to its own rows of device input buffer
        `buf` (uploaded ahead on the copy stream, or copied now), then the round's frames are made ONE contiguous range:
        the rows themselves where they already are one (every lane but the last with a full window, neighbours, one
        buffer), else gathered into the round buffer by device-to-device copies.  -> (buffer index or None = gathered,
        first row, frames)."""
        for s, buf, n in requests:
            lane = self.lanes[s]
            if lane._up_ahead[buf] == n:
                self.ctx.stream.wait_event(self._up_events[s][buf])
            else:
                self._upload_lane(s, buf, n)
            lane._up_ahead[buf] = 0
        total = sum(n for _, _, n in requests)
        contiguous = len({buf for _, buf, _ in requests}) == 1 and all(
            requests[i + 1][0] == requests[i][0] + 1 and requests[i][2] == self.W for i in range(len(requests) - 1))
        if contiguous:
            return requests[0][1], requests[0][0] * self.W, total
        pos = 0
        for s, buf, n in requests:
            self._gather_lane(s, buf, n, pos)
            pos += n
        return None, 0, total


class MultiSequenceEngine(_MultiSequenceBase):
    """`lanes` SOS sequences of one rig through one SequenceEngine-like store: same keyword arguments as SequenceEngine.
    The store is sosvo_sequence_workspace(cfg, S W, S (2 W + 1)) with cfg.n_pairs = S W; lane s owns the slots
    s (2 W + 1) .. s (2 W + 1) + 2 W."""

    def __init__(self, ctx, model, rig, lanes=2, window=32, num_of_features=1000, kp_cap=None, frame_cap=2048, median_win_size=11,
                 quality=0.01, min_distance=5.0, edge=31, thr=None, max_iter=210, adaptive=True, lm_iter=30,
                 ransac_solver="GP3P", detection_method="GFT", cross_check_stereo=False, cross_check_f2f=False,
                 gated_stereo=False, gated_f2f=False, gated_max_distance=None, ratio_stereo=False, ratio_f2f=False, ratio=None,
                 subpix=None, f2f_tracker="match", lk=None, stereo_refine=None, stereo_lk=None, cyclic_columns=False):
        so = StepOptions.of(cross_check_stereo, cross_check_f2f, gated_stereo, gated_f2f, gated_max_distance, ratio_stereo,
                            ratio_f2f, ratio, subpix, f2f_tracker, lk, stereo_refine, stereo_lk, cyclic_columns, rig,
                            store_levels=LK_MAX_LEVELS, detection_method=detection_method, edge=edge)
        self._init_lanes(lanes, window)
        self._adopt(_OmniFamily(ctx, model, rig, self.window, self.slots, True, so, num_of_features=num_of_features, kp_cap=kp_cap,
                                frame_cap=frame_cap, median_win_size=median_win_size, quality=quality, min_distance=min_distance,
                                edge=edge, thr=thr, max_iter=max_iter, adaptive=adaptive, lm_iter=lm_iter,
                                ransac_solver=ransac_solver, detection_method=detection_method))


class RGBDMultiSequenceEngine(_MultiSequenceBase):
    """`lanes` RGB-D sequences of one camera through one store: same keyword arguments as RGBDSequenceEngine; the lanes'
    push_window() takes (bgr, depth) tuples."""

    def __init__(self, ctx, cam, lanes=2, window=32, image_shape=(480, 640), num_of_features=1000, kp_cap=None, frame_cap=None,
                 median_win_size=0, quality=0.01, min_distance=5.0, edge=31, thr=None, max_iter=210, adaptive=True, lm_iter=30,
                 mask=None, pose_est_algorithm="EPNP", detection_method="GFT", cross_check=False, gated_f2f=False,
                 gated_max_distance=None, ratio_f2f=False, ratio=None, f2f_tracker="match", lk=None, stereo_refine=None,
                 stereo_lk=None, cyclic_columns=False):
        so = StepOptions.rgbd(cross_check, gated_f2f, gated_max_distance, ratio_f2f, ratio, f2f_tracker, lk, stereo_refine, stereo_lk,
                              cyclic_columns)      # (a tracker, a stereo refinement, cyclic columns: ValueError)
        self._init_lanes(lanes, window)
        self._adopt(_RGBDFamily(ctx, cam, self.window, self.slots, True, so, mask,
                                image_shape=image_shape, num_of_features=num_of_features, kp_cap=kp_cap,
                                frame_cap=frame_cap, median_win_size=median_win_size, quality=quality, min_distance=min_distance,
                                edge=edge, thr=thr, max_iter=max_iter, adaptive=adaptive, lm_iter=lm_iter,
                                pose_est_algorithm=pose_est_algorithm, detection_method=detection_method))


def dense_mask(ctx, model):
    """The top view's unwrapped annulus mask [rows, cols] u8 of a DeviceImageModel (1 = valid): a pixel is valid where unwrapping
    an all-255 frame gives 255.  Made once per model."""
    if getattr(model, "_dense_mask", None) is None:
        if getattr(model, "unwrap_table", None) is None:  # once per model
            model.unwrap_table = ctx.unwrap_prepare(model.omni_masks, model.map_x, model.map_y, (model.H, model.W))
        white = torch.full((1, model.H, model.W, 3), 255, dtype=torch.uint8, device=ctx.device)
        gray = ctx.unwrap_median_gray(white, model.unwrap_table, 0)
        model._dense_mask = (gray[0] == 255).to(torch.uint8).contiguous()
        ctx.synchronize()      # (engines on other streams that share the model find it ready)
    return model._dense_mask


class DenseOmniStereo(object):
    """Dense omnistereo for n_frames frames at once: OmniStereoModel.get_depth_map_from_panoramas
    (camera_models.py:3395) + triangulate_from_depth_map (:2567) as a batched device stage.  step() runs unwrap_median_gray
    through the model's table, Context.dense_stereo between the top and the bottom gray panoramas under the top view's
    annulus mask, and Context.dense_triangulate: three asynchronous C-ABI calls on one stream.
    options: a DenseOptions (None: the defaults).  min_disparity / max_disparity (rows): the reference's two filters of
    resolve_pano_correspondences_from_disparity_map, applied by the triangulation (max_disparity <= 0: no upper one).
    speckle: what SpeckleOptions.of takes.  None: no filter, and nothing differs from an engine without
    the argument.  With a value step() filters d16 in place (Context.dense_speckle) between the stereo and the triangulation,
    so that the returned map, X and depth() are the filtered ones.
    paths: 4, or 8 for the diagonal aggregation paths as well, the reference tuner's "Full DP"
    trackbar: paths = 8 if tuner.full_dyn_prog else 4.  With 4 nothing differs from an engine without the argument.
    wls: what WlsOptions.of takes, the tuner's "Use WLS filter" / "WLS lambda" / "WLS sigma" through
    WlsOptions.from_tuner.  None: no filter, and nothing differs from an engine without the argument.  With a value step() runs
    dense_filter.dense_confidence and dense_filter.dense_wls on d16, guided by the top gray panoramas under the engine's mask,
    in place, after the stereo and the speckle filter and before the triangulation.
    disparities: the number of disparities searched from options.min_disparity on, a multiple of 16 in 16 .. 256 (DESIGN.md
    section 42), the reference tuner's num_of_disparities: disparities = tuner.num_of_disparities.  With 64 nothing differs from
    an engine without the argument; every other value runs dense_wide.dense_stereo in place of Context.dense_stereo, and the
    speckle filter, the WLS filter and the triangulation follow unchanged."""

    def __init__(self, ctx, model, rig, n_frames, median_win_size=0, options=None, min_disparity=1.0, max_disparity=0.0,
                 speckle=None, paths=4, wls=None, disparities=64):
        from ._lib import DENSE_DISPARITIES, DenseOptions, SpeckleOptions, WlsOptions, dense_disparities, dense_paths
        self.options, self.speckle, self.wls = DenseOptions.of(options), SpeckleOptions.of(speckle), WlsOptions.of(wls)
        self.paths = dense_paths(paths, self.options)
        self.disparities = dense_disparities(disparities, self.paths, self.options)
        self._wide = self.disparities != DENSE_DISPARITIES
        self.ctx, self.model, self.rig_cfg, self.rig = ctx, model, rig, rig.as_struct()
        if tuple(rig.pano_top) != tuple(rig.pano_bot):
            raise ValueError("dense stereo needs two panoramas of one geometry, got %r and %r" % (rig.pano_top, rig.pano_bot))
        self.F, self.median_win_size = int(n_frames), int(median_win_size)
        self.min_disparity, self.max_disparity = float(min_disparity), float(max_disparity)
        self.mask = dense_mask(ctx, model)
        dev = ctx.device
        self.omni = torch.zeros((self.F, model.H, model.W, 3), dtype=torch.uint8, device=dev)
        self.gray = torch.zeros((2 * self.F, model.rows, model.cols), dtype=torch.uint8, device=dev)
        self.d16 = self.X = None

    def load_frames(self, omni):
        t = torch.from_numpy(np.ascontiguousarray(omni)) if isinstance(omni, np.ndarray) else omni
        self.omni.copy_(t.to(self.ctx.device))

    def step(self):
        """-> (d16 [F,rows,cols] i16, X [F,rows,cols,3] f64) on the device (asynchronous)."""
        c, m = self.ctx, self.model
        c.unwrap_median_gray(self.omni, m.unwrap_table, self.median_win_size, gray=self.gray)
        if self._wide:
            from . import dense_wide
            self.d16 = dense_wide.dense_stereo(c, self.gray[:self.F], self.gray[self.F:], self.mask, options=self.options,
                                               disparities=self.disparities, paths=self.paths)
        else:
            self.d16 = c.dense_stereo(self.gray[:self.F], self.gray[self.F:], self.mask, options=self.options, paths=self.paths)
        if self.speckle is not None:
            c.dense_speckle(self.d16, options=self.speckle, out=self.d16)
        if self.wls is not None:
            from . import dense_filter
            self.conf = dense_filter.dense_confidence(c, self.d16, options=self.wls)   # (kept: the step is asynchronous)
            dense_filter.dense_wls(c, self.d16, self.gray[:self.F], options=self.wls, conf=self.conf, mask=self.mask, out=self.d16)
        self.X = c.dense_triangulate(self.rig, self.d16, self.min_disparity, self.max_disparity)
        return self.d16, self.X

    def depth(self):
        """|X - F_top| as f32 [F,rows,cols] of the last step (NaN where invalid), by torch on the device."""
        F_top = torch.from_numpy(np.asarray(self.rig_cfg.F_top, np.float64).reshape(3)).to(self.ctx.device)
        return torch.linalg.vector_norm(self.X - F_top, dim=-1).to(torch.float32)
