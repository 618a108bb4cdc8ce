"""The ray-cast scene of DESIGN.md section 42 -- a room whose walls stand nearer than 64 disparities reach -- for
tests/test_dense_wide_reference.py, tests/test_gpu_dense_wide.py and scripts/bench_dense_wide.py, rendered once per process.  No
GPU and no test module here."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refdense  # noqa: E402

_SCENE = {}


def near_room_scene():
    """The scene of DESIGN.md section 42: synthetic_gums(), Panorama(width=1440) (146 rows), Room(seed=3, half_x=(250, 400),
    half_y=(300, 1000), cells=(60, 15)), pose t = 0, noise 2, the CPU oracle's unwrap, no median -> (gs, omni, the two gray
    panoramas, the two views' masks, the ray-cast disparity)."""
    if "scene" not in _SCENE:
        import oracle
        from vo_single_camera_sos_amd import synthetic
        from vo_single_camera_sos_amd.omnistereo.gum import synthetic_gums
        from vo_single_camera_sos_amd.omnistereo.panorama import Panorama
        gs = synthetic_gums()
        for m in (gs.top_model, gs.bot_model):
            m.panorama = Panorama(m, width=1440)
        gs.make_annulus_masks((480, 640))
        room = synthetic.Room(seed=3, half_x=(250.0, 400.0), half_y=(300.0, 1000.0), cells=(60.0, 15.0))
        t = np.zeros(3)
        omni = synthetic.render_omni(gs, room, np.eye(3), t, 2.0, np.random.default_rng(1))
        white = np.full_like(omni, 255)
        gray, valid = [], []
        for m in (gs.top_model, gs.bot_model):
            mx, my = m.panorama.float32_maps()
            gray.append(oracle.median_gray(oracle.unwrap(omni, m.mask, mx, my), 0))
            valid.append(oracle.median_gray(oracle.unwrap(white, m.mask, mx, my), 0) == 255)
        _SCENE["scene"] = (gs, omni, gray, valid, refdense.true_disparity(gs, room, t))
    return _SCENE["scene"]
