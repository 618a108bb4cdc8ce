"""run_VO's frame loop without a GPU: the per-frame path (frame_window 0) on a scripted tracker and scripted frames
(cfg_fakes.ScriptedRig / ScriptedTracker / ScriptedFrame).  What each run writes -- the three .txt files, printed_messages.log
and stdout, without the "Avg Time" lines (process time) and with the results directory written as <results> -- is compared
byte for byte with tests/golden/vo_loop_scripted/<run>/, which this module wrote with the loop as it was before it was taken
apart (python tests/test_vo_loop_scripted.py writes them again).

The runs reach every branch of the loop:
    default     no ground truth, a thread name; default thresholds: both metrics below their thresholds, translation in band,
                both above their maxima, in band with too few tracked correspondences, in band with too few keypoints, rotation
                alone in band (with the default thresholds: the "CRAZYNESS" line, dist < pos_max < ang_max is false), translation
                in band with the rotation beyond its maximum ("CRAZYNESS" again), a tracking failure that ends the run
    files       frames read from image files by position, a ground-truth file shorter than the sequence (the nan lines), a model
                with T_Cest_wrt_Rgt
    live        _keyframe_thresholds as run_VO_live passes them, ground truth present and shorter (a live run: identity):
                rotation alone in band makes a keyframe"""
import contextlib
import io
import os

import numpy as np
import pytest

import cfg_fakes
from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet
from vo_single_camera_sos_amd.omnistereo import transformations as tr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vo_loop_scripted")
FILES = ("estimated_frame_poses_TUM.txt", "gt_associated_frame_poses_TUM.txt", "keyframe_ids.txt", "printed_messages.log", "stdout.txt")
LIVE_THRESHOLDS = (0.05, 0.50, np.deg2rad(5.0), np.deg2rad(60.0))     # (run_VO_live's)


def _T(t, deg, axis=(0.0, 0.0, 1.0)):
    T = tr.rotation_matrix(np.deg2rad(deg), axis)
    T[:3, 3] = t
    return T


# (T_frame_wrt_tracking_ref_frame [m], num_tracked_correspondences, inlier ratio, num_valid_keypoints, True or the failure message)
SCRIPTS = {
    "default": [
        (None, 0, 0., 400, True),
        (_T((0.004, 0.0, 0.003), 0.2), 300, 0.90, 390, True),                    # both below their thresholds
        (_T((0.05, -0.01, 0.0), 0.5), 280, 0.85, 380, True),                     # translation in band
        (_T((0.3, 0.0, 0.1), 15.0), 200, 0.70, 370, True),                       # both above their maxima
        (_T((0.05, 0.0, 0.0), 0.5), 10, 0.30, 360, True),                        # in band, too few tracked correspondences
        (_T((0.06, 0.0, 0.0), 0.5), 200, 0.60, 30, True),                        # in band, too few keypoints
        (_T((0.001, 0.0, 0.0), 5.0, (0.0, 1.0, 0.0)), 210, 0.65, 350, True),     # rotation alone in band
        (_T((0.0, 0.1, 0.0), 12.0, (1.0, 0.0, 0.0)), 220, 0.75, 340, True),      # translation in band, rotation beyond its maximum
        (_T((0.0, -0.02, 0.1), 3.0, (1.0, 1.0, 0.0)), 230, 0.80, 330, True),     # translation in band again
        (_T((0.002, 0.0, 0.0), 0.1), 240, 0.95, 320, True),
        (None, 0, 0., 310, "Cannot track on only 3 point correspondences")],
    "files": [
        (None, 0, 0., 500, True),
        (_T((0.0, 0.03, 0.0), 0.3), 400, 0.9, 480, True),
        (_T((0.001, 0.0, 0.0), 0.1), 390, 0.8, 470, True),
        (_T((0.0, 0.0, -0.12), 2.0, (0.0, 1.0, 0.0)), 380, 0.7, 460, True),
        (_T((0.25, 0.0, 0.0), 0.0), 370, 0.6, 450, True)],
    "live": [
        (None, 0, 0., 600, True),
        (_T((0.01, 0.0, 0.0), 10.0), 500, 0.9, 590, True),                       # rotation alone in band: a keyframe
        (_T((0.2, 0.0, 0.1), 1.0), 480, 0.8, 580, True),                         # translation in band
        (_T((0.01, 0.0, 0.0), 1.0), 460, 0.7, 570, True),                        # both below
        (_T((0.03, 0.0, 0.0), 2.0), 440, 0.6, 560, True),                        # in the default band, below the live one
        (_T((0.3, 0.0, 0.0), 70.0), 420, 0.5, 550, True),                        # translation in band, rotation beyond its maximum
        (_T((0.0, 0.0, 0.0), 30.0, (0.0, 1.0, 0.0)), 400, 0.4, 540, True)],
}
GT_LINES = ["# index tx ty tz qx qy qz qw   [m]"] + [
    "%d %.9f %.9f %.9f 0.0 0.0 %.9f %.9f" % (i, 0.01 * i, -0.02 * i, 0.005 * i, np.sin(0.025 * i), np.cos(0.025 * i)) for i in range(4)]
FILE_INDICES = [0, 2, 3, 5, 6]      # positions among seven image files; the ground truth has poses 0 .. 3


def run_scripted(name, tmp_path, monkeypatch):
    """-> ({file name: text}, run_VO's dict) of the run `name`."""
    from vo_single_camera_sos_amd.omnistereo.common_cv import imwrite
    monkeypatch.setattr(pet, "TrackerStereoSE3", cfg_fakes.ScriptedTracker)
    monkeypatch.setattr(pet, "StereoPanoramicFrame", cfg_fakes.ScriptedFrame)
    results = str(tmp_path / ("results_" + name))
    gt = str(tmp_path / "gt_TUM.txt")
    with open(gt, "w") as f:
        f.write("\n".join(GT_LINES) + "\n")
    script = SCRIPTS[name]
    stdout = io.StringIO()
    if name == "default":
        rig = cfg_fakes.ScriptedRig(script)
        with pytest.warns(UserWarning, match="T1: Warning failed: Cannot track on only 3 point correspondences"), \
                contextlib.redirect_stdout(stdout):
            out = pet.run_VO(None, rig, results_path=results, thread_name="T1", frame_window=0,
                             _live_frames=lambda: ((k, None, None) for k in range(len(script))))
    elif name == "files":
        os.makedirs(str(tmp_path / "img"), exist_ok=True)
        for k in range(7):
            imwrite(str(tmp_path / "img" / ("image-%04d.png" % k)), np.full((2, 2, 3), k, np.uint8))
        rig = cfg_fakes.ScriptedRig(script, T_Cest_wrt_Rgt=_T((100.0, 0.0, 50.0), -90.0, (1.0, 0.0, 0.0)))     # [mm], the rig's units
        with contextlib.redirect_stdout(stdout):
            out = pet.run_VO(None, rig, gt_poses_filename=gt, img_filename_template=str(tmp_path / "img" / "image-*.png"),
                             img_indices=FILE_INDICES, results_path=results, frame_window=0)
    else:
        rig = cfg_fakes.ScriptedRig(script)
        with contextlib.redirect_stdout(stdout):
            out = pet.run_VO(None, rig, gt_poses_filename=gt, results_path=results, frame_window=0, _keyframe_thresholds=LIVE_THRESHOLDS,
                             _live_frames=lambda: ((k, None, None) for k in range(len(script))))
    texts = {"stdout.txt": stdout.getvalue()}
    for f in FILES[:4]:
        with open(os.path.join(results, f)) as fh:
            texts[f] = fh.read()
    where = os.path.realpath(results)
    return {f: "".join(line for line in t.replace(where, "<results>").splitlines(True) if "Avg Time" not in line)
            for f, t in texts.items()}, out


def golden(name, f):
    with open(os.path.join(GOLDEN, name, f)) as fh:
        return fh.read()


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_scripted_run_writes_the_recorded_files(name, tmp_path, monkeypatch):
    texts, out = run_scripted(name, tmp_path, monkeypatch)
    assert sorted(texts) == sorted(FILES)
    for f in FILES:
        assert texts[f] == golden(name, f), (name, f)
    n = len(SCRIPTS[name]) - (name == "default")      # (the failed frame is not written)
    assert len(out["poses"]) == n and out["tracked"] == n - 1 and "sequence_mode" not in out
    assert "".join("%d\n" % k for k in out["keyframe_ids"]) == texts["keyframe_ids.txt"]
    assert out["message"].splitlines()[0] in texts["stdout.txt"]


def test_the_recorded_files_hold_every_branch():
    """The fixtures themselves: each branch of the loop left its line (a script that no longer reaches one is noticed here)."""
    log, out = golden("default", "printed_messages.log"), golden("default", "stdout.txt")
    assert log.count("as Keyframe due to translation") == 2 and log.count("CRAZYNESS") == 2 and log.count("doesn't satisfy") == 2
    assert "Cannot track on only 3 point correspondences" in log and "Cannot track" not in out
    assert log.replace("Cannot track on only 3 point correspondences\n", "") == out
    assert golden("default", "keyframe_ids.txt") == "0\n2\n8\n"
    assert golden("default", "gt_associated_frame_poses_TUM.txt").splitlines()[3] == "3 0.0 0.0 0.0 0.0 0.0 0.0 1.0"
    gt = golden("files", "gt_associated_frame_poses_TUM.txt").splitlines()
    assert [line.split()[0] for line in gt] == [str(i) for i in FILE_INDICES]
    assert gt[3] == "5 nan nan nan nan nan nan nan" and gt[4] == "6 nan nan nan nan nan nan nan" and "nan" not in "".join(gt[:3])
    live = golden("live", "printed_messages.log")
    assert "as Keyframe due to  rotation: 0.17 > 0.09 [radians]" in live and live.count("CRAZYNESS") == 1
    assert golden("live", "gt_associated_frame_poses_TUM.txt").splitlines()[5] == "5 0.0 0.0 0.0 0.0 0.0 0.0 1.0"


DEFAULT_THRESHOLDS = (0.01, 0.20, np.deg2rad(1.0), np.deg2rad(10.0))
# (run, frame, dist [m], ang [deg], n_tracked, tracked_prev_avg, M_F, M_K, tracked_wrt_keyframe) -> create (and the frame's
# line in the run's log)
POLICY_TABLE = [
    ("default", 1, 0.005, 0.2, 150.0, 0.0, 390, 400, 1, False),             # both below their thresholds: nothing is said
    ("default", 2, 0.0509901951359, 0.5, 140.0, 150.0, 380, 400, 2, True),  # translation in band
    ("default", 3, 0.316227766, 15.0, 100.0, 0.0, 370, 380, 1, False),      # both above their maxima
    ("default", 4, 0.05, 0.5, 5.0, 100.0, 360, 380, 2, False),              # too few tracked correspondences
    ("default", 5, 0.06, 0.5, 100.0, 52.5, 30, 380, 3, False),              # too few keypoints
    ("default", 6, 0.001, 5.0, 105.0, 68.33, 350, 380, 4, False),           # rotation alone, default thresholds: CRAZYNESS
    ("default", 7, 0.1, 12.0, 110.0, 77.5, 340, 380, 5, False),             # translation in band, rotation beyond its maximum
    ("default", 8, 0.10198039027, 3.0, 115.0, 84.0, 330, 380, 6, True),
    ("live", 1, 0.01, 10.0, 250.0, 0.0, 590, 600, 1, True),                 # rotation alone, live thresholds: a keyframe
    ("live", 2, 0.2236067977, 1.0, 240.0, 0.0, 580, 590, 1, True),
    ("live", 4, 0.03, 2.0, 220.0, 230.0, 560, 580, 2, False),               # in the default band, below the live one
    ("live", 5, 0.3, 70.0, 210.0, 225.0, 550, 580, 3, False),
    ("live", 6, 0.0, 30.0, 200.0, 220.0, 540, 580, 4, True),
]


@pytest.mark.parametrize("row", POLICY_TABLE, ids=lambda r: "%s-%d" % r[:2])
def test_keyframe_policy_table(row):
    """The policy alone, on the figures the scripted runs put into it: the same decision, and the message is the line the
    whole loop wrote for that frame (none where it wrote none)."""
    run, idx, dist, deg, n_tracked, prev_avg, M_F, M_K, since_kf, create = row
    prefix = "T1: " if run == "default" else ""
    got = pet.keyframe_policy(dist, np.deg2rad(deg), n_tracked, prev_avg, M_F, M_K,
                              DEFAULT_THRESHOLDS if run == "default" else LIVE_THRESHOLDS, prefix, idx, since_kf)
    said = [line for line in golden(run, "printed_messages.log").splitlines() if line.startswith("%sFrame [%d] " % (prefix, idx))]
    assert got == (create, said[0] if said else None) and len(said) <= 1
    assert (idx in [int(k) for k in golden(run, "keyframe_ids.txt").split()]) == create


def test_keyframe_policy_condition_as_written_in_the_reference():
    """dist < pos_max < ang_max decides the rotation branch: with the default thresholds 0.20 < 0.1745 is false, so a rotation
    alone never makes a keyframe there."""
    args = (0.001, np.deg2rad(5.0), 100.0, 0.0, 300, 300)
    assert pet.keyframe_policy(*args, DEFAULT_THRESHOLDS, "", 3, 1) == \
        (False, "Frame [3] as failed to create Keyframe due to some CRAZYNESS")
    assert pet.keyframe_policy(*args, (0.01, 0.17, np.deg2rad(1.0), np.deg2rad(10.0)), "", 3, 1) == \
        (True, "Frame [3] as Keyframe due to  rotation: 0.09 > 0.02 [radians]... with 100 tracked keypoint correspondences "
               "after tracking 1 frames")


if __name__ == "__main__":      # write the fixtures again (from the repository's root: python tests/test_vo_loop_scripted.py)
    import tempfile
    from pathlib import Path
    for run in sorted(SCRIPTS):
        with tempfile.TemporaryDirectory() as d, pytest.MonkeyPatch.context() as mp:
            got, _ = run_scripted(run, Path(d), mp)
        os.makedirs(os.path.join(GOLDEN, run), exist_ok=True)
        for fname, text in got.items():
            with open(os.path.join(GOLDEN, run, fname), "w") as fh:
                fh.write(text)
        print("wrote", run)
