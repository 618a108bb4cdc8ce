"""ORACLE -- TEST INFRASTRUCTURE ONLY.

The detection part of the reference's control flow restated on the oracle: one omni view (unwrap, median, gray, GFT / ORB /
FAST / AGAST per azimuthal mask, ORB descriptors) and one RGB-D frame (median, gray, whole-image detection, descriptors,
depth back-projection, range filter).  tests/refflow.py builds the stereo / tracking flow on these, and
scripts/fuzz_parity.py calls them directly, so that the suite and the fuzzer check against one flow.  Each function cites
the reference lines it follows; the arithmetic is the oracle's (oracle/*.c).
"""
import numpy as np

import oracle


def fast_keypoints(gray, mask_bits, which, thr=10):
    """cv2.FastFeatureDetector_create() (threshold 10, NMS, TYPE_9_16).detect(gray, mask): corner score > 0, strictly
    greater than the 8 neighbours, mask set; raster order -> [n,2] float32 (x, y)."""
    s = oracle.fast_score_map(gray, thr).astype(np.int32)
    keep = s > 0
    pad = np.pad(s, 1)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if dy == 1 and dx == 1:
                continue
            keep &= pad[dy:dy + s.shape[0], dx:dx + s.shape[1]] < s
    keep &= ((mask_bits >> which) & 1).astype(bool)
    ys, xs = np.nonzero(keep)
    return np.stack([xs, ys], axis=1).astype(np.float32)


def agast_keypoints(gray, mask_bits, which, thr=10):
    """cv2.AgastFeatureDetector_create() (threshold 10, NMS, OAST_9_16).detect(gray, mask): the FAST-9/16 corner set with
    AGAST's block-maximum suppression (oracle.agast_nms), mask set; raster order -> [n,2] float32 (x, y)."""
    keep = oracle.agast_nms(oracle.fast_score_map(gray, thr)) & ((mask_bits >> which) & 1).astype(bool)
    ys, xs = np.nonzero(keep)
    return np.stack([xs, ys], axis=1).astype(np.float32)


def detect_view(im, omni, view):
    """set_current_omni_image (camera_models.py:3107) + detect_sparse_features_on_panorama with GFT
    (camera_models.py:1708-1797) for one mirror: lists over azimuthal masks of keypoints / descriptors."""
    pano = oracle.unwrap(omni, im.omni_masks[view], im.map_x[view], im.map_y[view])  # :3114 + panorama.py:293
    gray = oracle.median_gray(pano, im.median_ksize)                                  # :1711, :1714
    if im.method == "ORB":                                                            # :1640, :1755, :1765
        kps, descs = [], []
        for kp4, _ in oracle.orb_detect(gray, im.mask_bits[view], im.nmask, im.max_corners, im.kp_cap):
            d, kept = oracle.orb_describe_levels(gray, kp4, im.pattern)
            kps.append(np.ascontiguousarray(kp4[kept][:, :2]))
            descs.append(d)
        return kps, descs, pano, gray
    blurred = oracle.gauss7(gray)
    kps, descs = [], []
    if im.method in ("FAST", "AGAST"):                                                # :1664-1671, :1755, :1765
        detect = fast_keypoints if im.method == "FAST" else agast_keypoints
        for m in range(im.nmask):
            kp = detect(gray, im.mask_bits[view], m)[: im.kp_cap]
            d, kept = oracle.orb_describe(blurred, kp, im.cos_a, im.sin_a, im.pattern, im.edge)
            kps.append(kp[kept])
            descs.append(d)
        return kps, descs, pano, gray
    eig = oracle.min_eigen(gray)
    for m in range(im.nmask):                                                         # :1730
        kp, _ = oracle.gft_select(eig, im.mask_bits[view], m, im.quality, im.min_distance, im.max_corners,
                                  cand_cap=oracle.gft_cand_cap(im.kp_cap))  # :1739 (the GPU selection's candidate limit)
        kp = kp[: im.kp_cap]                     # the selection stops at the capacity: its first kp_cap acceptances
        d, kept = oracle.orb_describe(blurred, kp, im.cos_a, im.sin_a, im.pattern, im.edge)                 # :1765
        kps.append(kp[kept])
        descs.append(d)
    return kps, descs, pano, gray


def rgbd_frame(cam, bgr, depth, max_corners, pattern, cos_a, sin_a, median_ksize=0, quality=0.01, min_distance=5.0,
               edge=31, mask=None, method="GFT", kp_cap=None):
    """RGBDFrame.establish_keypoints (pose_est_tools.py:600-623) with the GFT, ORB, FAST or AGAST detector (:477-516, :544,
    :547) and ORB descriptors (:553) on the oracle -> dict(m [M,2] f32, d [M,32] u8, X [M,3], b [M,3], n_kp).  kp_cap: the
    keypoint capacity per frame of the GPU front end (None: no cut for GFT / FAST / AGAST; ORB needs it, as its retainBest
    is cut inside the detector).  With GFT it also implies the candidate limit of the GPU selection (oracle.gft_cand_cap)."""
    method = method.upper()
    gray = oracle.median_gray(bgr, median_ksize)                                     # :528, :531
    mb = np.ones(gray.shape, np.uint32) if mask is None else (np.asarray(mask) != 0).astype(np.uint32)
    if method == "ORB":                                                              # :478, :547, :553
        kp4, _ = oracle.orb_detect(gray, mb, 1, max_corners, kp_cap)[0]
        d, kept = oracle.orb_describe_levels(gray, kp4, pattern)
        kp = np.ascontiguousarray(kp4[kept, :2])
    else:
        if method in ("FAST", "AGAST"):                                              # :506-509
            kp = (fast_keypoints if method == "FAST" else agast_keypoints)(gray, mb, 0)
        else:
            kp, _ = oracle.gft_select(oracle.min_eigen(gray), mb, 0, quality, min_distance, max_corners,   # :544
                                      cand_cap=oracle.gft_cand_cap(kp_cap) if kp_cap else 0)
        kp = kp[:kp_cap]
        d, kept = oracle.orb_describe(oracle.gauss7(gray), kp, cos_a, sin_a, pattern, edge)            # :553
        kp = kp[kept]
    u, v = kp[:, 0].astype(np.uint64).astype(np.int32), kp[:, 1].astype(np.uint64).astype(np.int32)  # :611 (truncation)
    xyz, b = oracle.rgbd_backproject(depth, u, v, cam.intr, cam.depth_is_Z)          # camera_models.py:835-860
    Z = xyz[:, 2]
    valid = ~np.isnan(Z)                                                             # :613
    az = np.abs(np.nan_to_num(Z))                                                    # :583-584 on the Z row
    if cam.min_range > 0:
        valid &= az >= cam.min_range
    if cam.max_range > 0:
        valid &= az <= cam.max_range
    return dict(m=kp[valid].astype(np.float32), d=d[valid], X=xyz[valid], b=b[valid], n_kp=len(kp))
