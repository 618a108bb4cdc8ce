"""The scenes, the settings and the drivers every option's tests share (test infrastructure, like refflow.py and
refmatch.py): the calibrated rig, the rendered omni and RGB-D pairs with the reference flow under a setting, the translating
and the turning scene of the *_layers modules, the synthetic sequences behind run_VO, descriptor / position stores for the
stage tests -- and the plumbing of the chain every option is tested through: the one-call batch's records (batch_records,
pair_record), a sequence engine's speculative records (hop_records), a VO loop on one engine (drive) and on the lanes of a
multi-sequence engine (drive_lanes, assert_same_drive), run_VO over several frame windows (run_vo_windows) and run_VO_many
against solo runs (run_vo_many_against_solo).  The drivers return data; what it has to equal is asserted by the test that
makes the claim.

The scene builders memoise per (ctx, parameters) -- ctx is the session's context -- so the modules that ask for the same scene
share one rendering, one oracle detection and one cache of references, keyed by the matchers' VALUES (refmatch.Matching).
Nobody writes into a scene."""
import os
import threading

import numpy as np

import refflow
from refmatch import Matching, gate_matrix, two_smallest_keys

FILES = ("estimated_frame_poses_TUM.txt", "keyframe_ids.txt")
FX = FY = 554.256258
CX, CY = 319.5, 239.5
N_SEQ = 6
THR = float(1.0 - np.cos(np.deg2rad(5.0)))                    # the reference's 5-degree threshold
# the *_layers modules' settings (test_gpu_stereo_lk_layers passes its own 330 / 2048 / 500)
NFEAT, FRAME_CAP, ITERS = 300, 1024, 210
KW = dict(num_of_features=NFEAT, frame_cap=FRAME_CAP, max_iter=ITERS)
SEQ_KW = dict(KW, adaptive=True, ransac_solver="GP3P")
LK_CHECKED = dict(half=4, levels=3, max_iter=10, fb_max=0.5)      # 16 lanes per keypoint, forward-backward check
LK_WAVE = dict(half=10, levels=2, max_iter=10)                    # the whole-wave mapping, no check
_memo = {}


# ---- the setting -------------------------------------------------------------------------------------------------------------
def _switches(value):
    """A switch in run_VO's spelling -> (static stereo, frame to frame)."""
    return {None: (False, False), False: (False, False), True: (True, True), "both": (True, True), "stereo": (True, False),
            "f2f": (False, True)}[value]


class Setting(object):
    """The matcher options of one test case.  gate, ratio, cc: each option's switch in run_VO's spelling (None, False, True,
    "both", "stereo", "f2f"), handed to run_VO as spelt; cap: gated_max_distance; r: the ratio in 64ths, or None."""

    def __init__(self, name="off", gate=None, ratio=None, cc=None, cap=None, r=None):
        self.name, self.gate, self.ratio, self.cc, self.cap, self.r = name, gate, ratio, cc, cap, r
        (self.gate_stereo, self.gate_f2f), (self.ratio_stereo, self.ratio_f2f) = _switches(gate), _switches(ratio)
        self.cc_stereo, self.cc_f2f = _switches(cc)
        self.changes_stereo = self.gate_stereo or self.ratio_stereo or self.cc_stereo
        self.ratio_only = not (self.gate or self.cc) and bool(self.ratio)

    def _ratio(self):
        return None if self.r is None else self.r / 64.0

    def omni_kw(self):
        return dict(ratio_stereo=self.ratio_stereo, ratio_f2f=self.ratio_f2f, ratio=self._ratio(), gated_stereo=self.gate_stereo,
                    gated_f2f=self.gate_f2f, gated_max_distance=self.cap, cross_check_stereo=self.cc_stereo,
                    cross_check_f2f=self.cc_f2f)

    def rgbd_kw(self):
        return dict(ratio_f2f=self.ratio_f2f, ratio=self._ratio(), gated_f2f=self.gate_f2f, gated_max_distance=self.cap,
                    cross_check=self.cc_f2f)

    def run_vo_kw(self):
        return dict(ratio_test=self.ratio or None, ratio=self._ratio(), gated_matching=self.gate or None,
                    gated_max_distance=self.cap, cross_check=self.cc or None)

    def matchings(self):
        """-> (the static-stereo matcher, the frame-to-frame matcher) for refflow."""
        return tuple(Matching(gated=g, cap=self.cap if g else None, mutual=c, ratio=self.r if x else 0) for g, c, x in
                     zip(_switches(self.gate), _switches(self.cc), _switches(self.ratio)))


# ---- small helpers -----------------------------------------------------------------------------------------------------------
def dev(ctx, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def record(w):
    """The [16] record of a refflow track."""
    out = np.zeros(16)
    out[:12] = np.asarray(w["T"]).reshape(12)
    out[12], out[13] = w["ransac"]["n_inliers"], len(w["corr"]["cam"] if "cam" in w["corr"] else w["corr"]["q"])
    out[14], out[15] = w["ransac"]["status"], w["ransac"]["best_iter"]
    return out


def read_results(results, files=FILES):
    return tuple(open(os.path.join(results, f)).read() for f in files)


def sos_kwargs(seq, n, results):
    return dict(gt_poses_filename=os.path.join(seq, "omni", "gt_TUM.txt"), img_filename_template=os.path.join(seq, "omni", "image-*.png"),
                img_indices=list(range(n)), results_path=results)


def rgbd_kwargs(seq, n, results):
    d = os.path.join(seq, "rgbd")
    return dict(gt_poses_filename=os.path.join(d, "gt_TUM.txt"), img_filename_template=os.path.join(d, "rgb", "*.png"),
                depth_filename_template=os.path.join(d, "depth", "*.png"), img_indices=list(range(n)), results_path=results)


def rig():
    from vo_single_camera_sos_amd.omnistereo.gum import synthetic_gums
    from vo_single_camera_sos_amd.omnistereo.panorama import Panorama
    gs = synthetic_gums()
    for m in (gs.top_model, gs.bot_model):
        m.panorama = Panorama(m, width=1200)
    gs.make_annulus_masks((480, 640))
    pano = gs.top_model.panorama
    geo = (pano.cols, pano.rows, pano.pixel_size, pano.cyl_height_max)
    rig_kw = dict(pano_top=geo, pano_bot=geo, F_top=gs.top_model.F[:3, 0], F_bot=gs.bot_model.F[:3, 0], min_range=500.0,
                  max_range=7000.0, stereo_min_disp=1.0, stereo_max_hdiff=2.5, f2f_max_hdiff=0.125 * 0.5 * pano.cols,
                  pct_good_matches=1.0)
    return gs, rig_kw


def write_sos_sequences(root, seeds=(77, 61), frames=N_SEQ):
    """One synthetic SOS sequence per seed under root (steps |t| <= 40 mm, <= 2 degrees); frames: one count, or one per seed.
    -> their directories.  Rendered once per (seeds, frames): while those directories exist a later call returns them, so
    whoever writes into a sequence's directory asks for a combination of its own."""
    from vo_single_camera_sos_amd import synthetic
    counts = (frames,) * len(seeds) if isinstance(frames, int) else tuple(frames)
    key = ("sos", tuple(seeds), counts)
    if key not in _memo or not all(os.path.isdir(seq) for seq in _memo[key]):
        gs, _ = rig()
        _memo[key] = [os.path.join(str(root), "seq_%d" % k) for k in range(len(seeds))]
        for seq, seed, n in zip(_memo[key], seeds, counts):
            synthetic.write_sos_sequence(seq, gs, n_frames=n, seed=seed, max_t=40.0, max_deg=2.0)
    return list(_memo[key])


def drive(eng, frames, window):
    """What a VO loop asks of an engine: windows of frames; frame 0 becomes the keyframe, every later frame is also
    tracked serially against the keyframe slot.  -> per frame (count, seed, spec, spec2, serial record)."""
    out = []
    for w0 in range(0, len(frames), window):
        for i, info in enumerate(eng.push_window(list(frames[w0:w0 + window]))):
            rec = None
            if w0 + i == 0:
                eng.promote(info["slot"])
            else:
                rec = eng.track(eng.key_slot, info["slot"], info["seed"])
            out.append((info["count"], info["seed"], info["spec"], info["spec2"], rec))
    return out


def drive_lanes(multi, sequences, window):
    """sequences[k] through lane k of the multi-sequence engine, one host thread each, as run_VO_many drives them.  Every lane
    is live before the first one parks, so the rounds are in lockstep.  -> per lane what drive() returns.  A lane's exception
    is raised (the first lane's that has one) once every lane has been ended and joined."""
    S = len(sequences)
    got, errors = [None] * S, [None] * S

    def work(k):
        try:
            got[k] = drive(multi.lane(k), sequences[k], window)
        except BaseException as e:  # noqa: B902
            errors[k] = e
        finally:
            multi.end(k)
    for k in range(S):
        multi.begin(k)
    threads = [threading.Thread(target=work, args=(k,)) for k in range(S)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for e in errors:
        if e is not None:
            raise e
    return got


def assert_same_drive(got, want):
    """Two results of drive() are the same: as many frames, count and seed equal, the two speculative records and the serial
    record both None or equal bit for bit."""
    assert len(got) == len(want), (len(got), len(want))
    for t, (g, w) in enumerate(zip(got, want)):
        assert g[:2] == w[:2], (t, g[:2], w[:2])
        for x, y in zip(g[2:], w[2:]):
            assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), t


def hop_records(eng, frames, window):
    """The frames through a sequence engine window by window (the last one may be ragged; RGB-D: a list of (bgr, depth)
    tuples).  -> [len(frames) - 1, 16]: every frame's speculative record against its predecessor, in frame order."""
    got = []
    for w0 in range(0, len(frames), window):
        got += [info["spec"] for info in eng.push_window(list(frames[w0:w0 + window])) if info["spec"] is not None]
    return np.stack(got)


def batch_records(ctx, s, frames, seed=5, n_streams=1, fill=None, **kw):
    """The records of the frames' pairs from one FramePairBatch on the scene's model and rig (kw: its settings, the solver's
    among them); fill: a byte the workspace holds before the call."""
    from vo_single_camera_sos_amd.pipeline import FramePairBatch, RigConfig
    b = FramePairBatch(ctx, s["model"], RigConfig(**s["rig_kw"]), len(frames) // 2, seed=seed, n_streams=n_streams, **kw)
    if fill is not None:
        b.workspace.fill_(fill)
    b.load_frames(frames)
    out = b.step().cpu().numpy().copy()
    ctx.synchronize()
    return out


def pair_record(ctx, s, a, b, seed, **kw):
    """The pair batch's record of frames (a, b) of the scene's sequence, memoised per (scene, a, b, seed, settings): what
    the sequence tests compare against."""
    key = ("pair", ctx, s["name"], a, b, seed, repr(sorted(kw.items())))
    if key not in _memo:
        _memo[key] = batch_records(ctx, s, s["seq"][[a, b]], seed=seed, **kw)[0]
    return _memo[key]


def run_vo_windows(cam, seq, n, root, windows, **kw):
    """run_VO on the first n frames of the SOS sequence once per frame window (0: the per-frame mirror path), each into a
    directory of its own under root; every run tracks every frame.  -> (the result files' texts, run_VO's outputs), per window."""
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import run_VO
    texts, outs = {}, {}
    for w in windows:
        results = os.path.join(str(root), "window_%s" % w)
        outs[w] = run_VO(None, cam, frame_window=w, **kw, **sos_kwargs(seq, n, results))
        texts[w] = read_results(results)
        assert outs[w]["tracked"] == n - 1, (w, outs[w].get("message"))
    return texts, outs


def run_vo_many_against_solo(gums, sequences, n, root, frame_window=5, lanes=2, **kw):
    """The sequences through the lanes of one engine (run_VO_many) against each through run_VO alone: every sequence's
    result files are its solo run's, byte for byte.  -> (the solo runs' texts, run_VO_many's outputs), per sequence."""
    from vo_single_camera_sos_amd.omnistereo.gum import load_gums_json
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import run_VO, run_VO_many
    want = []
    for k, seq in enumerate(sequences):
        res = os.path.join(str(root), "solo_%d" % k)
        out = run_VO(None, load_gums_json(gums), frame_window=frame_window, **kw, **sos_kwargs(seq, n, res))
        assert out["tracked"] == n - 1, (k, out.get("message"))
        want.append(read_results(res))
    many = [sos_kwargs(seq, n, os.path.join(str(root), "many_%d" % k)) for k, seq in enumerate(sequences)]
    outs = run_VO_many(load_gums_json(gums), many, frame_window=frame_window, lanes=lanes, **kw)
    for k, (q, files) in enumerate(zip(many, want)):
        assert read_results(q["results_path"]) == files, k
    return want, outs


# ---- the scenes of the *_layers modules ------------------------------------------------------------------------------------------
def _yaw(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def translating_scene(ctx):
    """3 rendered pairs (seed 99: the first two are the pairs test_pair_pipeline_tracks_with_lk uses) with their poses, and a
    6-frame sequence with steps |t| <= 40 mm, <= 2 degrees.  Fewer pairs or frames of the same seeds are prefixes of these."""
    key = ("translating", ctx)
    if key not in _memo:
        from vo_single_camera_sos_amd import synthetic
        from vo_single_camera_sos_amd.frontend import DeviceImageModel
        gs, rig_kw = rig()
        omni, poses = synthetic.make_frame_pairs(gs, 3, seed=99)
        room, rng = synthetic.Room(seed=61), np.random.default_rng(62)
        seq = np.stack([synthetic.render_omni(gs, room, R, t, 2.0, rng) for R, t in synthetic.trajectory(6, 61, max_t=40.0, max_deg=2.0)])
        _memo[key] = dict(name="translating", gs=gs, rig_kw=rig_kw, omni=omni, poses=poses, seq=seq,
                          model=DeviceImageModel(ctx, gs, (480, 640)))
    return _memo[key]


def yaw_pairs(gs, yaw_deg, seeds=(5, 6)):
    """-> (omni [4, H, W, 3], poses): pair i = one room seen from the identity pose and from the pose turned by -/+ yaw_deg."""
    from vo_single_camera_sos_amd import synthetic
    omni, poses = [], []
    for k, seed in enumerate(seeds):
        rng = np.random.default_rng(seed)
        room = synthetic.Room(seed=seed)
        R = _yaw(yaw_deg if k else -yaw_deg)
        omni += [synthetic.render_omni(gs, room, np.eye(3), np.zeros(3), 2.0, rng), synthetic.render_omni(gs, room, R, np.zeros(3), 2.0, rng)]
        poses.append((R, np.zeros(3)))
    return np.stack(omni), poses


def turning_scene(ctx):
    """Per yaw angle (21 degrees: a matched pair can cross the seam; 11: a tracked point can) two rendered pairs whose second
    frame is the first turned about the vertical axis, as yaw_omni[yaw] and yaw_poses[yaw]; and a 6-frame sequence that turns
    by 7 degrees a frame about the vertical axis while it drifts 30 mm a frame."""
    key = ("turning", ctx)
    if key not in _memo:
        from vo_single_camera_sos_amd import synthetic
        from vo_single_camera_sos_amd.frontend import DeviceImageModel
        gs, rig_kw = rig()
        pairs = {yaw: yaw_pairs(gs, yaw) for yaw in (21.0, 11.0)}
        room, rng = synthetic.Room(seed=71), np.random.default_rng(72)
        seq = np.stack([synthetic.render_omni(gs, room, _yaw(7.0 * k), np.array([30.0 * k, -10.0 * k, 0.0]), 2.0, rng) for k in range(6)])
        _memo[key] = dict(name="turning", gs=gs, rig_kw=rig_kw, yaw_omni={yaw: p[0] for yaw, p in pairs.items()},
                          yaw_poses={yaw: p[1] for yaw, p in pairs.items()}, seq=seq, model=DeviceImageModel(ctx, gs, (480, 640)))
    return _memo[key]


# ---- the rendered omni pairs ---------------------------------------------------------------------------------------------------
class _OmniPairs(object):
    def __init__(self, ctx, B, black, solver):
        from vo_single_camera_sos_amd import orb_pattern, synthetic
        from vo_single_camera_sos_amd.frontend import DeviceImageModel, ImageFrontEnd
        self.B, self.nfeat, self.seed, self.solver, self.thr = B, 330, 5, dict(solver), THR
        gs, self.rig_kw = rig()
        self.omni, _ = synthetic.make_frame_pairs(gs, B, seed=99)
        for f in black:
            self.omni[f] = 0
        self.model = DeviceImageModel(ctx, gs, (480, 640))
        self.fe = ImageFrontEnd(ctx, self.model, 2 * B, detection_method="GFT", num_of_features=self.nfeat)
        self.fe.load_frames(self.omni)
        self.fe.run()
        ctx.synchronize()
        ca, sa = orb_pattern.angle_cos_sin(-1.0)
        im = refflow.ImageModel(self.model.map_x.cpu().numpy(), self.model.map_y.cpu().numpy(), self.model.omni_masks.cpu().numpy(),
                                self.model.mask_bits_host, 12, self.nfeat, orb_pattern.orb_pattern(), ca, sa, method="GFT",
                                kp_cap=self.fe.kp_cap)
        self.views = [[refflow.detect_view(im, self.omni[f], v)[:2] for v in range(2)] for f in range(2 * B)]
        self.rp = refflow.RigParams(**self.rig_kw)
        self._frames, self._tracks = {}, {}

    def frames(self, setting, pct=1.0):
        """refflow.stereo_frame of every frame under the setting (pct: the rig's pct_good_matches)."""
        key = (setting.matchings()[0], pct)
        if key not in self._frames:
            rp = refflow.RigParams(**dict(self.rig_kw, pct_good_matches=pct))
            self._frames[key] = [refflow.stereo_frame(rp, v[0][0], v[1][0], v[0][1], v[1][1], matching=key[0]) for v in self.views]
        return self._frames[key]

    def track(self, setting, a, b, seed, pct=1.0):
        """refflow.track_pair of frames (a, b) under the setting, with the scene's solver settings."""
        key = (setting.matchings(), pct, a, b, seed)
        if key not in self._tracks:
            frames, rp = self.frames(setting, pct), refflow.RigParams(**dict(self.rig_kw, pct_good_matches=pct))
            self._tracks[key] = refflow.track_pair(rp, frames[a], frames[b], self.thr, self.solver["max_iter"], seed=seed,
                                                   adaptive=self.solver.get("adaptive", False),
                                                   gp3p=self.solver.get("ransac_solver") == "GP3P", matching=key[0][1])
        return self._tracks[key]

    def pair_tracks(self, setting, pct=1.0):
        """What the pair paths compute: pair i = frames (2 i, 2 i + 1) with seed + i."""
        return [self.track(setting, 2 * i, 2 * i + 1, self.seed + i, pct) for i in range(self.B)]

    def hop_tracks(self, setting):
        """What the sequence engines speculate: frame t against t - 1 with seed t - 1."""
        return [self.track(setting, t - 1, t, t - 1) for t in range(1, 2 * self.B)]


def omni_pairs(ctx, B=2, black=(), solver=(("max_iter", 210), ("adaptive", True), ("ransac_solver", "GP3P"))):
    """B rendered pairs (seed 99, GFT 330 features; the frames in `black` zeroed): the front end on the GPU (.fe, .model), the
    detection on the oracle (.views), and the reference flow under a Setting (.frames, .track, ...).  solver: the trackers'
    keyword values (.solver) -- by default generalised P3P, 210 iterations with the adaptive stop, so that one reference
    serves the pair paths and the sequence engines."""
    key = ("omni", ctx, B, tuple(black), tuple(solver))
    if key not in _memo:
        _memo[key] = _OmniPairs(ctx, B, black, solver)
    return _memo[key]


# ---- the rendered RGB-D pairs ----------------------------------------------------------------------------------------------------
class _RGBDPairs(object):
    def __init__(self):
        from vo_single_camera_sos_amd import orb_pattern, synthetic
        from vo_single_camera_sos_amd.pipeline import RGBDCamConfig
        self.B, self.nfeat, self.thr = 2, 1000, THR
        yaw = np.deg2rad(40.0)
        R_yaw = np.array([[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
        bgr, depth = [], []
        for i in range(self.B):
            rng = np.random.default_rng(900 + i)
            room = synthetic.Room(seed=900 + i, half_x=(1800.0, 2600.0), half_y=(2500.0, 3500.0), cells=(150.0, 40.0))
            R, t = synthetic.random_step(rng, max_t=80.0, max_deg=8.0)
            for (Rw, tw) in ((R_yaw, np.zeros(3)), (R_yaw @ R, R_yaw @ t)):
                im, dp = synthetic.render_rgbd(room, Rw, tw, rng, FX, FY, CX, CY, depth_is_Z=True)
                bgr.append(im)
                depth.append(dp)
        self.bgr, self.depth = np.stack(bgr), np.stack(depth)
        self.cam = RGBDCamConfig(fx=FX, fy=FY, center_x=CX, center_y=CY, depth_is_Z=True, min_range=0.8, max_range=7.0)
        self.kw = dict(num_of_features=self.nfeat, max_iter=210, adaptive=True, pose_est_algorithm="EPNP")
        ca, sa = orb_pattern.angle_cos_sin(orb_pattern.GFT_KEYPOINT_ANGLE)
        self.rc = refflow.RGBDParams(FX, FY, CX, CY, self.cam.focal_length_m, True, 0.8, 7.0, self.cam.f2f_max_hdiff, 1.0)
        self.frames = [refflow.rgbd_frame(self.rc, self.bgr[f], self.depth[f], self.nfeat, orb_pattern.orb_pattern(), ca, sa)
                       for f in range(2 * self.B)]
        self._tracks = {}

    def track(self, setting, a, b, seed):
        """refflow.track_pair_rgbd of frames (a, b) under the setting (None: plain refflow), with the solver settings of .kw."""
        key = (setting and setting.matchings()[1], a, b, seed)
        if key not in self._tracks:
            self._tracks[key] = refflow.track_pair_rgbd(self.rc, self.frames[a], self.frames[b], self.thr, 210, seed=seed,
                                                        adaptive=True, epnp=True, matching=key[0])
        return self._tracks[key]


def rgbd_pairs(ctx):
    """2 rendered RGB-D pairs (1000 GFT features) with their oracle frames (.frames) and the reference flow under a Setting."""
    key = ("rgbd", ctx)
    if key not in _memo:
        _memo[key] = _RGBDPairs()
    return _memo[key]


# ---- descriptor / position stores for the stage tests ------------------------------------------------------------------------------
def descriptor_scene(rng, blocks, stride, counts, u_span=40.0, v_span=12.0):
    """A descriptor / position store: every block re-observes block 0's first rows with 0-6 flipped bits at a position
    jittered by a few pixels (distinctive matches), some rows are copies of each other (ties), the rest is random."""
    desc = rng.integers(0, 256, (blocks, stride, 32), dtype=np.uint8)
    pos = np.stack([rng.uniform(0, u_span, (blocks, stride)), rng.uniform(0, v_span, (blocks, stride))], -1).astype(np.float32)
    n0 = max(1, int(counts[0]))
    for b in range(blocks):
        n = int(counts[b])
        for i in range(0, n, 2):
            src = int(rng.integers(0, n0))
            d = desc[0, src].copy()
            for bit in rng.integers(0, 256, rng.integers(0, 7)):
                d[bit >> 3] ^= np.uint8(1 << (bit & 7))
            desc[b, i] = d
            pos[b, i] = pos[0, src] + rng.uniform(-3.0, 3.0, 2).astype(np.float32)
        for i in range(5, n, 11):
            desc[b, i] = desc[b, i - 3]
    return desc, pos


class StageProblems(object):
    """One set of matching problems on the device, optionally through slot tables over the stores; the two smallest keys of
    the definition are computed once per (blocks, gate, direction)."""

    def __init__(self, ctx, qd, td, qp, tp, nq, nt, q_slot=None, t_slot=None):
        self.ctx, self.qd, self.td, self.qp, self.tp, self.nq, self.nt = ctx, qd, td, qp, tp, nq, nt
        self.P = len(nq) if q_slot is None else len(q_slot)
        self.qs = np.arange(self.P) if q_slot is None else q_slot
        self.ts = np.arange(self.P) if t_slot is None else t_slot
        self.d_qd, self.d_td, self.d_qp, self.d_tp = [dev(ctx, a) for a in (qd, td, qp, tp)]
        self.d_nq, self.d_nt = dev(ctx, nq.astype(np.int32)), dev(ctx, nt.astype(np.int32))
        self.sl = {} if q_slot is None else dict(q_slot=dev(ctx, q_slot.astype(np.int32)), t_slot=dev(ctx, t_slot.astype(np.int32)))
        self.cache = {}

    def smallest(self, p, gate, reverse):
        """(k1, k2) of problem p over the trains admissible under gate = (min_dv, max_du) or None."""
        qs, ts = int(self.qs[p]), int(self.ts[p])
        sig = (qs, ts, gate, reverse and gate is not None)
        if sig not in self.cache:
            n, m = min(int(self.nq[qs]), self.qd.shape[1]), min(int(self.nt[ts]), self.td.shape[1])
            adm = None if gate is None else gate_matrix(self.qp[qs, :n], self.tp[ts, :m], gate[0], gate[1], reverse)
            self.cache[sig] = two_smallest_keys(self.qd[qs, :n], self.td[ts, :m], adm)
        return self.cache[sig]

