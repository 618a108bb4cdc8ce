"""Host-side mirror of the helpers of omnistereo/common_cv.py on either side of the hot path: the pixel gates
(numpy, as in the reference; the batched pipeline applies the same gates inside the assembly kernels) and the
sequence readers of the VO loop (image list, BGR image, 16-bit depth PNG) -- on Pillow, cv2 does not exist here."""
import fnmatch
import os

import numpy as np


def get_images(filename_template, indices_list=(), show_images=False, return_names_only=False):
    """common_cv.py:1293-1352: the files matching `filename_template` (directory + fnmatch pattern), optionally
    sub-selected by position.  The listing is SORTED here (the reference takes os.listdir order, which is
    arbitrary)."""
    path_to_files, pattern = os.path.split(filename_template)
    names = sorted(fnmatch.filter(os.listdir(path_to_files), pattern))
    all_names = [os.path.join(path_to_files, n) for n in names]
    if indices_list is None or len(indices_list) == 0:
        indices_list = range(len(all_names))
    selected = [all_names[i] for i in indices_list]
    if return_names_only:
        return selected
    return [imread(fn) for fn in selected]


def imread(filename):
    """cv2.imread(filename): uint8 [rows, cols, 3] in B, G, R order (None when unreadable)."""
    from PIL import Image
    try:
        with Image.open(filename) as im:
            rgb = np.asarray(im.convert("RGB"))
    except (OSError, ValueError):
        return None
    return np.ascontiguousarray(rgb[..., ::-1])


def imwrite(filename, bgr_or_gray):
    from PIL import Image
    a = np.asarray(bgr_or_gray)
    Image.fromarray(a[..., ::-1] if a.ndim == 3 else a).save(filename)


def get_depthmap_float32_from_png(depth_img_filename, conversion_factor=1.0):
    """common_cv.py:2150-2158: the 16-bit depth PNG times the conversion factor, as float32."""
    from PIL import Image
    with Image.open(depth_img_filename) as im:
        raw = np.asarray(im)
    return np.float32(conversion_factor * raw)


def filter_pixel_correspondences(matched_points_top, matched_points_bot, min_rectified_disparity, max_horizontal_diff):
    """common_cv.py:167-188: |u_top - u_bot| <= max_horizontal_diff (if > 0) and v_top - v_bot >=
    min_rectified_disparity (if >= 0), both limits inclusive -> bool array."""
    matched_points_top = np.asarray(matched_points_top)
    matched_points_bot = np.asarray(matched_points_bot)
    if max_horizontal_diff > 0:
        validation_hor_diff = np.abs(matched_points_top[..., 0] - matched_points_bot[..., 0]) <= max_horizontal_diff
    else:
        validation_hor_diff = np.ones(shape=(matched_points_top.shape[:-1]), dtype="bool")
    if min_rectified_disparity >= 0:
        validation_min_disparity = matched_points_top[..., 1] - matched_points_bot[..., 1] >= min_rectified_disparity
        return np.logical_and(validation_hor_diff, validation_min_disparity)
    return validation_hor_diff


def calc_optical_flow_pyr_lk(prev_gray, next_gray, prev_pts, next_pts=None, win_half=10, max_level=2, max_iter=30, eps=0.01,
                             min_eig_threshold=1e-4, ctx=None, cyclic=False):
    """cv2.calcOpticalFlowPyrLK(prevImg, nextImg, prevPts, nextPts, winSize=(2 win_half + 1,) * 2, maxLevel=max_level,
    criteria=(COUNT + EPS, max_iter, eps), minEigThreshold=min_eig_threshold), the call the reference carries commented out
    at camera_models.py:3070, with cv2's shapes and the arithmetic on the GPU (Context.gray_pyramid + Context.track_lk: the
    integer restatement of include/sosvo.h, replicated borders).  prev_gray, next_gray: [rows, cols] u8 of one size;
    prev_pts: [N, 1, 2] or [N, 2] float32; next_pts: the starting guesses (OPTFLOW_USE_INITIAL_FLOW) or None
    -> (next_pts [N, 1, 2] float32, status [N, 1] uint8, err [N, 1] float32).  More than 4096 points go in chunks.
    cyclic: the images are full-circle panoramas, column `cols` is column 0 again (SOSVO_LK_CYCLIC_COLUMNS: no cv2
    counterpart); cols must be a multiple of 2^max_level and the top level at least 2 win_half + 3 columns wide."""
    import torch
    from .. import _lib
    from ..runtime import default_context
    c = default_context() if ctx is None else ctx
    prev_gray, next_gray = np.ascontiguousarray(prev_gray), np.ascontiguousarray(next_gray)
    if prev_gray.dtype != np.uint8 or prev_gray.ndim != 2 or next_gray.dtype != np.uint8 or next_gray.shape != prev_gray.shape:
        raise ValueError("prev_gray / next_gray: two uint8 images [rows, cols] of one size")
    pts = np.ascontiguousarray(prev_pts, dtype=np.float32).reshape(-1, 2)
    guess = None if next_pts is None else np.ascontiguousarray(next_pts, dtype=np.float32).reshape(-1, 2)
    if guess is not None and guess.shape != pts.shape:
        raise ValueError("next_pts: one starting guess per point")
    opts = _lib.LKOptions(half=win_half, levels=max_level + 1 if isinstance(max_level, int) else max_level,
                          max_iter=max_iter, eps=eps, min_eig=min_eig_threshold)
    if cyclic and (prev_gray.shape[1] % (1 << (opts.levels - 1)) or (prev_gray.shape[1] >> (opts.levels - 1)) < 2 * opts.half + 3):
        raise ValueError("cyclic: a width of %d columns is no multiple of %d, or its top level is narrower than the %d-column "
                         "template" % (prev_gray.shape[1], 1 << (opts.levels - 1), 2 * opts.half + 3))
    N = len(pts)
    out = (np.zeros((N, 1, 2), np.float32), np.zeros((N, 1), np.uint8), np.zeros((N, 1), np.float32))
    if N == 0:
        return out
    dev = c.device
    pyr = (c.gray_pyramid_cyclic if cyclic else c.gray_pyramid)(torch.from_numpy(np.stack([prev_gray, next_gray])).to(dev), opts.levels)
    img0, img1 = torch.zeros((1,), dtype=torch.int32, device=dev), torch.ones((1,), dtype=torch.int32, device=dev)
    for lo in range(0, N, _lib.LK_MAX_CAP):
        hi = min(N, lo + _lib.LK_MAX_CAP)
        n = torch.full((1,), hi - lo, dtype=torch.int32, device=dev)
        g = None if guess is None else torch.from_numpy(guess[lo:hi]).to(dev).reshape(1, hi - lo, 2).contiguous()
        nx, st, er = c.track_lk(pyr, img0, img1, torch.from_numpy(pts[lo:hi]).to(dev).reshape(1, hi - lo, 2).contiguous(), n,
                                half=opts.half, max_iter=opts.max_iter, eps=opts.eps, min_eig=opts.min_eig, next_pts=g)
        out[0][lo:hi, 0], out[1][lo:hi, 0], out[2][lo:hi, 0] = nx[0].cpu().numpy(), st[0].cpu().numpy(), er[0].cpu().numpy()
    return out
