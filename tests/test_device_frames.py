"""The device-frame classes (DeviceStereoFrame / DeviceRGBDFrame) and the trackers' _track_device_frame on a fake engine: no
device.  The poses in tests/golden/vo_loop_scripted/track_device_frame.json are what the two per-family functions this one
replaced gave for the same records (python tests/test_device_frames.py writes the file from the functions as they are)."""
import json
import os

import numpy as np
import pytest

from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vo_loop_scripted", "track_device_frame.json")
FAMILIES = ("sos", "rgbd")


class _Cfg(object):
    median_ksize = 11


class _RigCfg(object):
    stereo_min_disp, stereo_max_hdiff, min_range, max_range = 1.0, 2.5, 500.0, 7000.0


class _CamCfg(object):
    min_range, max_range = 0.8, 7.0


class Engine(object):
    """What a device frame and _track_device_frame touch of a sequence engine; counts the reads of its configuration."""
    key_slot, rig_cfg, cam_cfg = 9, _RigCfg(), _CamCfg()

    def __init__(self, serial_record=None):
        self.cfg_reads, self.serial_record, self.track_calls, self.promoted = 0, serial_record, [], []

    @property
    def cfg(self):
        self.cfg_reads += 1
        return _Cfg()

    def track(self, key_slot, slot, seed):
        self.track_calls.append((key_slot, slot, seed))
        return self.serial_record

    def promote(self, slot):
        self.promoted.append(slot)


class _Model(object):
    def __init__(self, units):
        self.units = units


def _frame(family, engine, info, model=None, frame_id=5, seq_index=5, parent_id=3):
    if family == "sos":
        return pet.DeviceStereoFrame(engine, info, model or _Model("mm"), frame_id, seq_index, parent_id=parent_id)
    return pet.DeviceRGBDFrame(engine, info, model or _Model("m"), frame_id, seq_index, parent_id=parent_id)


def _tracker(family, T_key=None):
    cls = pet.TrackerStereoSE3 if family == "sos" else pet.TrackerRGBDSE3
    t = cls.__new__(cls)
    t.set_global_parameters_for_tracking()
    t.number_of_cams = 2 if family == "sos" else 1
    t.T_Ckey_wrt_S_est_list = [] if T_key is None else [T_key]
    t.num_tracked_correspondences, t.inlier_tracked_correspondences_ratio = 0, 0.
    return t


def _record(pose, inliers, matches):
    return np.concatenate([np.asarray(pose, dtype=np.float64).reshape(12), [inliers, matches, 0.0, 17.0]])


def _rot(deg, axis):
    from vo_single_camera_sos_amd.omnistereo.transformations import rotation_matrix
    return rotation_matrix(np.deg2rad(deg), axis)


# poses of the records: an ordinary one, and one with negative zeros in rotation and translation
POSE = _rot(3.0, (0.2, 1.0, -0.3))[:3].copy()
POSE[:, 3] = (12.5, -40.0, 3.25)
POSE_NEG_ZERO = np.array([[1.0, -0.0, 0.0, -0.0], [-0.0, -1.0, -0.0, 25.0], [0.0, -0.0, -1.0, -0.0]])
# keyframe poses to chain with: one with negative zeros of its own (where multiplying into an identity first could show)
T_KEY = _rot(-20.0, (1.0, 0.5, 0.0))
T_KEY[:3, 3] = (0.1, 0.2, -0.3)
T_KEY_NEG_ZERO = np.array([[-1.0, -0.0, -0.0, 0.5], [-0.0, 1.0, -0.0, -0.0], [-0.0, -0.0, -1.0, -0.0], [0.0, 0.0, 0.0, 1.0]])
CASES = {"plain": (POSE, T_KEY), "negative_zero_pose": (POSE_NEG_ZERO, T_KEY), "negative_zero_both": (POSE_NEG_ZERO, T_KEY_NEG_ZERO),
         "no_keyframe_pose": (POSE_NEG_ZERO, None)}


def _tracked_pose(family, case):
    pose, T_key = CASES[case]
    t, eng = _tracker(family, T_key), Engine()
    cur = _frame(family, eng, dict(slot=2, seed=4, count=300, spec=_record(pose, 150, 200)))
    ok, msg = t._track_device_frame(_frame(family, eng, dict(slot=1, seed=3, count=310, spec=None), seq_index=4), cur)
    assert ok and msg == "tracking used 150 inlier point correspondences"
    return t, cur


def _hex(a):
    return [float(v).hex() for v in np.asarray(a).reshape(-1)]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_chained_pose_is_the_replaced_functions_bit_for_bit(family, case):
    with open(GOLDEN) as f:
        want = json.load(f)[family][case]
    t, cur = _tracked_pose(family, case)
    assert _hex(t.T_C_curr_frame_wrt_S_est) == want["T_C_curr_frame_wrt_S_est"]          # (hex: signed zeros count)
    assert _hex(cur.T_frame_wrt_tracking_ref_frame) == want["T_frame_wrt_tracking_ref_frame"]
    k = 1e-3 if family == "sos" else 1.0                 # (the rig's millimetres become metres)
    assert np.array_equal(cur.T_frame_wrt_tracking_ref_frame[:3, 3], CASES[case][0][:, 3] * k)
    assert t.num_tracked_correspondences == 150 and t.inlier_tracked_correspondences_ratio == 0.75


@pytest.mark.parametrize("family", FAMILIES)
def test_record_selection(family):
    """The spec record against the predecessor, the spec2 record against the frame before it, else ONE serial call against
    the keyframe slot with the frame's slot and seed."""
    spec, spec2, serial = _record(POSE, 101, 200), _record(POSE, 102, 200), _record(POSE, 103, 200)
    eng = Engine(serial)
    cur = _frame(family, eng, dict(slot=6, seed=40, count=300, spec=spec, spec2=spec2), seq_index=8)
    for ref_seq, want, calls in ((7, 101, 0), (6, 102, 0), (5, 103, 1), (None, 103, 2)):
        t = _tracker(family)
        ref = object() if ref_seq is None else _frame(family, eng, dict(slot=0, seed=0, count=1, spec=None), seq_index=ref_seq)
        assert t._track_device_frame(ref, cur) == (True, "tracking used %d inlier point correspondences" % want)
        assert t.num_tracked_correspondences == want and len(eng.track_calls) == calls
    assert eng.track_calls == [(9, 6, 40), (9, 6, 40)]
    # without speculative records every reference takes the serial call
    eng2 = Engine(serial)
    bare = _frame(family, eng2, dict(slot=3, seed=41, count=300, spec=None), seq_index=8)
    for ref_seq in (7, 6):
        ref = _frame(family, eng2, dict(slot=0, seed=0, count=1, spec=None), seq_index=ref_seq)
        assert _tracker(family)._track_device_frame(ref, bare)[0]
    assert eng2.track_calls == [(9, 3, 41), (9, 3, 41)]


@pytest.mark.parametrize("family,least", [("sos", 4), ("rgbd", 6)])
def test_minimum_number_of_matches(family, least):
    """SOS: 2 * 3 * (0.33 * 2) = 3.96; RGB-D: 2 * 3 * 1 = 6.  Below: refused before anything is kept."""
    eng = Engine()
    ref = _frame(family, eng, dict(slot=0, seed=0, count=1, spec=None), seq_index=4)
    t = _tracker(family)
    t.indices_inliers_combined = "kept"
    cur = _frame(family, eng, dict(slot=1, seed=1, count=50, spec=_record(POSE, 3, least - 1)))
    assert t._track_device_frame(ref, cur) == (False, "Cannot track on only %d point correspondences" % (least - 1))
    assert t.num_tracked_correspondences == 0 and t.indices_inliers_combined == "kept"
    assert cur.T_frame_wrt_tracking_ref_frame is not None and np.array_equal(cur.T_frame_wrt_tracking_ref_frame, np.identity(4))
    cur = _frame(family, eng, dict(slot=1, seed=1, count=50, spec=_record(POSE, 3, least)))
    assert t._track_device_frame(ref, cur) == (True, "tracking used 3 inlier point correspondences")
    assert t.num_tracked_correspondences == 3 and t.inlier_tracked_correspondences_ratio == 3.0 / least
    # the inlier list stays on the device: SOS forgets the host path's, the RGB-D tracker has no such attribute to reset
    assert t.indices_inliers_combined == (None if family == "sos" else "kept")


def test_no_model_is_refused_by_the_rgbd_tracker_only():
    """Fewer inliers than the model needs: RGB-D reports the frame as not tracked (after the counts are kept), SOS has no
    such check."""
    rec = _record(POSE, 2, 40)
    eng = Engine()
    t = _tracker("rgbd", T_KEY)
    cur = _frame("rgbd", eng, dict(slot=1, seed=1, count=50, spec=rec))
    assert t._track_device_frame(_frame("rgbd", eng, dict(slot=0, seed=0, count=1, spec=None), seq_index=4), cur) == \
        (False, "RANSAC (EPNP) found no model among 40 correspondences")
    assert t.num_tracked_correspondences == 2 and t.inlier_tracked_correspondences_ratio == 0.05
    assert np.array_equal(cur.T_frame_wrt_tracking_ref_frame, np.identity(4))
    t = _tracker("sos", T_KEY)
    cur = _frame("sos", eng, dict(slot=1, seed=1, count=50, spec=rec))
    assert t._track_device_frame(_frame("sos", eng, dict(slot=0, seed=0, count=1, spec=None), seq_index=4), cur) == \
        (True, "tracking used 2 inlier point correspondences")


SOS_ATTRIBUTES = dict(
    panoramic_image_top=None, panoramic_image_bottom=None, use_midpoint_triangulation=True, use_opengv_triangulation=False,
    first_row_to_crop_bottom=0, total_time=0., pano_correspondences=None, conversion_factor_length_to_m=0.001, median_win_size=11,
    min_disp=1.0, max_u_dist=2.5, min_range=500.0, max_range=7000.0, frame_id=12, parent_id=10, slot=3, seq_index=7, seed=6,
    num_valid_keypoints=321)
RGBD_ATTRIBUTES = dict(
    frame_id=12, parent_id=10, conversion_factor_length_to_m=1.0, total_time=0., median_win_size=11, min_range=0.8, max_range=7.0,
    mask=None, rgb_img=None, depth_map=None, current_depth=None, keypoints_and_descriptors=None, bearing_vectors=None,
    keypoints_3D_points=None, slot=3, seq_index=7, seed=6, num_valid_keypoints=321)


@pytest.mark.parametrize("family", FAMILIES)
def test_attributes_of_a_device_frame(family):
    """vars(frame): the names and values the keyframe classes copy blindly; the per-engine constants are built once."""
    eng, model = Engine(), _Model("mm" if family == "sos" else "m")
    spec, spec2 = _record(POSE, 1, 2), _record(POSE, 3, 4)
    info = dict(slot=np.int64(3), seed=np.int32(6), count=np.int64(321), spec=spec, spec2=spec2)
    f = _frame(family, eng, info, model, frame_id=12, seq_index=np.int64(7), parent_id=10)
    want = dict(SOS_ATTRIBUTES if family == "sos" else RGBD_ATTRIBUTES)
    got = dict(vars(f))
    assert got.pop("engine") is eng and got.pop("spec_record") is spec and got.pop("spec2_record") is spec2
    if family == "rgbd":
        assert got.pop("rgbd_camera_model") is model
    T = got.pop("T_frame_wrt_tracking_ref_frame")
    assert T.dtype == np.float64 and np.array_equal(T, np.identity(4))
    assert got == want and {k: type(v) for k, v in got.items()} == {k: type(v) for k, v in want.items()}
    # a record without spec2 (a window's first frame), no parent: spec2_record None, parent_id -1
    g = (pet.DeviceStereoFrame if family == "sos" else pet.DeviceRGBDFrame)(eng, dict(slot=0, seed=1, count=2, spec=None), model, 13, 8)
    assert g.spec2_record is None and g.spec_record is None and g.parent_id == -1 and sorted(vars(g)) == sorted(vars(f))
    assert eng.cfg_reads == 1                      # (ctypes field reads are slow: once per engine, not per frame)
    g.promote()
    f.promote()
    assert eng.promoted == [0, 3]
    # the keyframe classes take a device frame's attributes as they are
    kf = (pet.StereoPanoramicKeyFrame if family == "sos" else pet.RGBDKeyFrame)(frame=f)
    assert {k: v for k, v in vars(kf).items() if k != "children_ids"} == vars(f) and kf.children_ids == []
    assert isinstance(f, pet.StereoPanoramicFrame if family == "sos" else pet.RGBDFrame)


if __name__ == "__main__":      # write the recorded poses again (from the repository's root: python tests/test_device_frames.py)
    out = {}
    for fam in FAMILIES:
        out[fam] = {}
        for name in sorted(CASES):
            tracker, frame = _tracked_pose(fam, name)
            out[fam][name] = dict(T_C_curr_frame_wrt_S_est=_hex(tracker.T_C_curr_frame_wrt_S_est),
                                  T_frame_wrt_tracking_ref_frame=_hex(frame.T_frame_wrt_tracking_ref_frame))
    with open(GOLDEN, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", GOLDEN)
