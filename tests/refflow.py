"""The reference's per-frame / per-pair control flow restated on top of the CPU oracle (test
infrastructure; also the `cpu_baseline` leg of bench.py).  Each function cites the reference lines
it follows; the arithmetic is the oracle's (oracle/*.c)."""
import numpy as np

import oracle
# the detection flows (omni views, RGB-D frames) live in oracle/flow.py, where scripts/fuzz_parity.py reads them too
from oracle.flow import agast_keypoints, detect_view, fast_keypoints, rgbd_frame  # noqa: F401

IDX = 0xFFFFF


class RigParams(object):
    """Constants of one calibrated rig (host floats), mirrors struct sosvo_rig."""

    def __init__(self, pano_top, pano_bot, F_top, F_bot, min_range, max_range, stereo_min_disp=1.0,
                 stereo_max_hdiff=2.5, f2f_max_hdiff=-1.0, pct_good_matches=1.0):
        self.pano_top, self.pano_bot = tuple(pano_top), tuple(pano_bot)  # (cols, rows, pixel_size, h_max)
        self.F_top, self.F_bot = np.asarray(F_top, np.float64), np.asarray(F_bot, np.float64)
        self.min_range, self.max_range = min_range, max_range
        self.stereo_min_disp, self.stereo_max_hdiff = stereo_min_disp, stereo_max_hdiff
        self.f2f_max_hdiff, self.pct_good_matches = f2f_max_hdiff, pct_good_matches


def match_sorted(query_desc, train_desc):
    """FeatureMatcher.match (camera_models.py:404-446): 1-NN then stable sort by distance.
    -> (query_idx, train_idx, dist) in sorted order."""
    if len(query_desc) == 0 or len(train_desc) == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z
    keys = oracle.match_hamming(query_desc, train_desc, k=1)[:, 0]
    order = oracle.sort_matches(keys)
    return order.astype(np.int64), (keys[order] & IDX).astype(np.int64), (keys[order] >> 20).astype(np.int64)


def stereo_frame(rig, kp_top, kp_bot, desc_top, desc_bot, *, matching=None):
    """match_features_panoramic_top_bottom (camera_models.py:3027-3101) followed by
    establish_stereo_correspondences (pose_est_tools.py:339-397).  kp_* / desc_*: lists over buckets of
    [n,2] float32 / [n,32] uint8.  -> dict of arrays in the reference's order.
    matching: None for the reference's matcher, or the step's matcher under other options: a callable (query_desc, train_desc,
    query_pos, train_pos, gate) -> match_sorted's triple, gate = the step's pixel gate (min_dv, max_du), with an attribute
    `gated` (tests/refmatch.py).  A gated one has searched under the gate already, so the gate below passes all it sees."""
    mt, mb, dt, db = [], [], [], []
    n_cand = 0
    for kt, kb, et, eb in zip(kp_top, kp_bot, desc_top, desc_bot):
        if len(kt) == 0 or len(kb) == 0:  # :3039
            continue
        if matching is None:
            q, t, _ = match_sorted(eb, et)  # query = bottom, train = top (:3042)
        else:
            q, t, _ = matching(eb, et, kb, kt, (rig.stereo_min_disp, rig.stereo_max_hdiff))
        good = int(rig.pct_good_matches * len(q))  # :3045
        q, t = q[:good], t[:good]
        n_cand += good
        mt.append(kt[t])
        mb.append(kb[q])
        dt.append(et[t])
        db.append(eb[q])
    if not mt:
        e2, e3, e32 = np.zeros((0, 2), np.float32), np.zeros((0, 3)), np.zeros((0, 32), np.uint8)
        return dict(m_top=e2, m_bot=e2, d_top=e32, d_bot=e32, X=e3, b_top=e3, b_bot=e3, n_cand=0)
    mt, mb = np.concatenate(mt).astype(np.float32), np.concatenate(mb).astype(np.float32)
    dt, db = np.concatenate(dt), np.concatenate(db)
    ok = oracle.pixel_gates(mt.astype(np.float64), mb.astype(np.float64), rig.stereo_min_disp,
                            rig.stereo_max_hdiff)  # :3086
    if matching is not None and matching.gated:
        assert ok.all()
    mt, mb, dt, db = mt[ok], mb[ok], dt[ok], db[ok]
    az1, el1 = oracle.pano_to_angles(mt[:, 0], mt[:, 1], *rig.pano_top)  # pose_est_tools.py:344
    az2, el2 = oracle.pano_to_angles(mb[:, 0], mb[:, 1], *rig.pano_bot)  # :345
    bt, bb = oracle.angles_to_bearing(az1, el1), oracle.angles_to_bearing(az2, el2)  # :348-349
    X = oracle.triangulate_midpoint(az1, el1, az2, el2, rig.F_top, rig.F_bot)  # :365
    good = oracle.range_filter_homo(X, rig.min_range, rig.max_range)  # :372
    return dict(m_top=mt[good], m_bot=mb[good], d_top=dt[good], d_bot=db[good], X=X[good], b_top=bt[good],
                b_bot=bb[good], n_cand=n_cand)


class ImageModel(object):
    """Per-model constants of the image front end (host arrays): float32 unwrap maps and annulus mask per
    view, azimuthal mask bit fields per view, detector settings."""

    def __init__(self, map_x, map_y, omni_masks, mask_bits, nmask, max_corners, pattern, cos_a, sin_a,
                 median_ksize=11, quality=0.01, min_distance=5.0, edge=31, method="GFT", kp_cap=1024):
        self.map_x, self.map_y, self.omni_masks, self.mask_bits = map_x, map_y, omni_masks, mask_bits
        self.nmask, self.max_corners, self.pattern = nmask, max_corners, pattern
        self.cos_a, self.sin_a = cos_a, sin_a
        self.median_ksize, self.quality, self.min_distance, self.edge = median_ksize, quality, min_distance, edge
        self.method, self.kp_cap = method.upper(), kp_cap


def frame_from_image(rig, im, omni):
    """StereoPanoramicFrame.__init__ for one omni image (pose_est_tools.py:271-402)."""
    kt, dt, _, _ = detect_view(im, omni, 0)
    kb, db, _, _ = detect_view(im, omni, 1)
    fr = stereo_frame(rig, kt, kb, dt, db)
    fr["n_kp_top"] = sum(len(k) for k in kt)
    fr["n_kp_bot"] = sum(len(k) for k in kb)
    return fr


def f2f_view(rig, m_train, d_train, m_query, d_query, *, matching=None):
    """match_features_frame_to_frame (pose_est_tools.py:211-269) for one view -> (train_idx, query_idx).
    matching: as in stereo_frame; its gate is off exactly when the view's own |du| gate is."""
    if matching is None:
        q, t, _ = match_sorted(d_query, d_train)  # query = current, train = reference (:215)
    else:
        q, t, _ = matching(d_query, d_train, np.asarray(m_query, np.float32)[:, :2], np.asarray(m_train, np.float32)[:, :2],
                           (-1.0, rig.f2f_max_hdiff if rig.f2f_max_hdiff >= 0 else -1.0))
    good = int(rig.pct_good_matches * len(q))  # :225
    q, t = q[:good], t[:good]
    if good > 0 and rig.f2f_max_hdiff >= 0:  # :245
        pt = np.zeros((good, 2))
        pq = np.zeros((good, 2))
        pt[:, 0] = m_train[t, 0]
        pq[:, 0] = m_query[q, 0]
        ok = oracle.pixel_gates(pt, pq, -1, rig.f2f_max_hdiff)  # :247
        if matching is not None and matching.gated:
            assert ok.all()
        q, t = q[ok], t[ok]
    return t, q


def track_inputs(rig, ref, cur, *, matching=None):
    """Correspondence stacking of TrackerStereoSE3.track_frame (pose_est_tools.py:741-778).
    ref / cur: dicts from stereo_frame.  -> f [n,3], p [n,3], cam [n], (q, t) index arrays, n_top."""
    t_top, q_top = f2f_view(rig, ref["m_top"], ref["d_top"], cur["m_top"], cur["d_top"], matching=matching)
    t_bot, q_bot = f2f_view(rig, ref["m_bot"], ref["d_bot"], cur["m_bot"], cur["d_bot"], matching=matching)
    f = np.vstack([cur["b_top"][q_top], cur["b_bot"][q_bot]])
    p = np.vstack([ref["X"][t_top], ref["X"][t_bot]])
    cam = np.concatenate([np.zeros(len(q_top), np.int32), np.ones(len(q_bot), np.int32)])
    return dict(f=f, p=p, cam=cam, q=np.concatenate([q_top, q_bot]), t=np.concatenate([t_top, t_bot]),
                n_top=len(q_top))


def track_pair(rig, ref, cur, thr, max_iter, seed, adaptive=False, lm_iter=30, gp3p=False, *, matching=None):
    """track_frame steps 3-4 (pose_est_tools.py:785, :830) on the oracle: RANSAC + LM on the inliers."""
    c = track_inputs(rig, ref, cur, matching=matching)
    cam_off = np.stack([rig.F_top, rig.F_bot])
    cam_rot = np.stack([np.eye(3), np.eye(3)])
    r = oracle.ransac_abs_pose(c["f"], c["p"], thr, max_iter, seed=seed, adaptive=adaptive, cam=c["cam"],
                               cam_off=cam_off, cam_rot=cam_rot, gp3p=gp3p)
    idx = np.nonzero(r["mask"])[0].astype(np.int32)
    T = r["T"]
    if r["status"] == 0:
        T, _, _ = oracle.refine_abs_pose(c["f"], c["p"], r["T"], idx=idx, cam=c["cam"], cam_off=cam_off,
                                         cam_rot=cam_rot, max_lm_iter=lm_iter)
    return dict(corr=c, ransac=r, T=T)


# ---- RGB-D (perspective) variant ---------------------------------------------------------------------------
class RGBDParams(object):
    """Host constants of the RGB-D path: RGBDCamModel (camera_models.py:756-779), RGBDFrame ranges
    (pose_est_tools.py:428-430) and the tracker's |du| gate (:958)."""

    def __init__(self, fx, fy, cx, cy, focal_length_m=1e-3, depth_is_Z=True, min_range=0.8, max_range=7.0,
                 f2f_max_hdiff=-1.0, pct_good_matches=1.0):
        self.intr = np.array([fx, fy, cx, cy, focal_length_m], dtype=np.float64)
        self.depth_is_Z, self.min_range, self.max_range = depth_is_Z, min_range, max_range
        self.f2f_max_hdiff, self.pct_good_matches = f2f_max_hdiff, pct_good_matches


def track_pair_rgbd(cam, ref, cur, thr, max_iter, seed, adaptive=False, lm_iter=30, epnp=True, gp3p=False, twopt=False, *,
                    matching=None):
    """TrackerRGBDSE3.track_frame (pose_est_tools.py:896-954) on the oracle: frame-to-frame matches, central
    RANSAC (:915), LM on the inliers (:937)."""
    t, q = f2f_view(cam, ref["m"], ref["d"], cur["m"], cur["d"], matching=matching)
    f, p = cur["b"][q], ref["X"][t]
    r = oracle.ransac_abs_pose(f, p, thr, max_iter, seed=seed, adaptive=adaptive, epnp=epnp, gp3p=gp3p, twopt=twopt)
    idx = np.nonzero(r["mask"])[0].astype(np.int32)
    T = r["T"]
    if r["status"] == 0:
        T, _, _ = oracle.refine_abs_pose(f, p, r["T"], idx=idx, max_lm_iter=lm_iter)
    return dict(corr=dict(f=f, p=p, q=q, t=t), ransac=r, T=T)


def pairs_worker(job):
    """One host process of the all-cores CPU baseline (bench.py): the whole reference flow on the oracle for a
    chunk of frame pairs.  job = (rig_kw, im_kw, omni [2n,H,W,3], thr, iters, seed0) -> seconds spent."""
    import time
    rig_kw, im_kw, omni, thr, iters, seed0 = job
    rp = RigParams(**rig_kw)
    im = ImageModel(**im_kw)
    t0 = time.perf_counter()
    for i in range(omni.shape[0] // 2):
        ref = frame_from_image(rp, im, omni[2 * i])
        cur = frame_from_image(rp, im, omni[2 * i + 1])
        track_pair(rp, ref, cur, thr, iters, seed=seed0 + i)
    return time.perf_counter() - t0


def pairs_records_worker(job):
    """As pairs_worker, but returns the [n,16] result records (3x4 refined pose, inliers, correspondences, status,
    winning iteration) -- tests/soak_parity.py compares them with the GPU's."""
    rig_kw, im_kw, omni, thr, iters, seed0 = job[:6]
    gp3p = bool(job[6]) if len(job) > 6 else False
    rp = RigParams(**rig_kw)
    im = ImageModel(**im_kw)
    out = np.zeros((omni.shape[0] // 2, 16))
    for i in range(omni.shape[0] // 2):
        ref = frame_from_image(rp, im, omni[2 * i])
        cur = frame_from_image(rp, im, omni[2 * i + 1])
        w = track_pair(rp, ref, cur, thr, iters, seed=seed0 + i, gp3p=gp3p)
        out[i, :12] = np.asarray(w["T"]).reshape(12)
        out[i, 12], out[i, 13] = w["ransac"]["n_inliers"], len(w["corr"]["cam"])
        out[i, 14], out[i, 15] = w["ransac"]["status"], w["ransac"]["best_iter"]
    return out


def rgbd_pairs_records_worker(job):
    """RGB-D counterpart of pairs_records_worker: job = (cam_kw, bgr [2n,...], depth [2n,...], nfeat, thr, iters, seed0,
    epnp) -> [n,16] records (tests/soak_parity.py --rgbd)."""
    from vo_single_camera_sos_amd import orb_pattern
    cam_kw, bgr, depth, nfeat, thr, iters, seed0, epnp = job
    cam = RGBDParams(**cam_kw)
    ca, sa = orb_pattern.angle_cos_sin(orb_pattern.GFT_KEYPOINT_ANGLE)
    pat = orb_pattern.orb_pattern()
    out = np.zeros((bgr.shape[0] // 2, 16))
    for i in range(bgr.shape[0] // 2):
        ref = rgbd_frame(cam, bgr[2 * i], depth[2 * i], nfeat, pat, ca, sa)
        cur = rgbd_frame(cam, bgr[2 * i + 1], depth[2 * i + 1], nfeat, pat, ca, sa)
        w = track_pair_rgbd(cam, ref, cur, thr, iters, seed=seed0 + i, epnp=epnp)
        out[i, :12] = np.asarray(w["T"]).reshape(12)
        out[i, 12], out[i, 13] = w["ransac"]["n_inliers"], len(w["corr"]["q"])
        out[i, 14], out[i, 15] = w["ransac"]["status"], w["ransac"]["best_iter"]
    return out
