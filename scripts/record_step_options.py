#!/usr/bin/env python
"""What the Python layers do with the step options, one outcome per case: a characterisation sweep over the public
constructors of pipeline.py (FramePairPipeline, OverlappedFramePairs, FramePairBatch, SequenceEngine, MultiSequenceEngine,
RGBDPairPipeline, RGBDPairBatch, RGBDSequenceEngine, RGBDMultiSequenceEngine), batch_cfg / rgbd_batch_cfg and run_VO's
_sos_engine_settings / _rgbd_engine_settings.  No GPU: device calls go to the recorder contexts of tests/test_lk_layers_cfg.py
and tests/test_stereo_lk_cfg.py and to the stand-ins of tests/cfg_fakes.py.

An outcome is either what the constructor raised (type and message, and what it had asked of its context by then) or: the
flags word, a hash of the configuration's bytes, the calls of one short drive, and .opts / .lk / .stereo_lk / .cyclic.  For
the engine settings: the keyword arguments and which of the sweep's cache keys compare equal.  Cases that break two rules at
once pin the ORDER of the checks.

    python scripts/record_step_options.py tests/golden/step_options_parent.json

writes the outcomes of the tree it is run from; tests/test_step_options.py recomputes them and compares.  The committed file
was written from the commit BEFORE the options became one value (_lib.StepOptions), by this script unchanged."""
import contextlib
import hashlib
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cfg_fakes  # noqa: E402
from test_lk_layers_cfg import SMALL, _drive, _model  # noqa: E402
from test_stereo_lk_cfg import _Rec  # noqa: E402
from vo_single_camera_sos_amd import _lib, frontend, pipeline  # noqa: E402
from vo_single_camera_sos_amd.omnistereo import pose_est_tools as pet  # noqa: E402

LK = dict(half=4, levels=2, max_iter=10, fb_max=0.5)
SLK = dict(half=3, max_iter=12, max_shift=1.5)
WIDTHS = (1200.0, 1204.0, 1200.5)      # the fakes' own width; no multiple of 8; no integer

# ---- the grids ---------------------------------------------------------------------------------------------------------------------
# (name, keyword arguments) of the omnistereo constructors; "W" cases are run at every width, the others at 1200
OMNI_PLAIN = [
    ("off", {}),
    ("cross_stereo", dict(cross_check_stereo=True)), ("cross_f2f", dict(cross_check_f2f=True)),
    ("gated_stereo", dict(gated_stereo=True)), ("gated_f2f_cap", dict(gated_f2f=True, gated_max_distance=64)),
    ("cap_alone", dict(gated_max_distance=64)), ("cap_300", dict(gated_f2f=True, gated_max_distance=300)),
    ("cap_300_alone", dict(gated_max_distance=300)),
    ("ratio_stereo", dict(ratio_stereo=True, ratio=0.75)), ("ratio_f2f", dict(ratio_f2f=True, ratio=0.75)),
    ("ratio_alone", dict(ratio=0.75)), ("ratio_missing", dict(ratio_f2f=True)), ("ratio_0.7", dict(ratio_stereo=True, ratio=0.7)),
    ("ratio_0.7_alone", dict(ratio=0.7)),
    ("subpix_2", dict(subpix=2)), ("subpix_5", dict(subpix=5)), ("subpix_true", dict(subpix=True)), ("subpix_false", dict(subpix=False)),
    ("subpix_6", dict(subpix=6)),
    ("match", dict(f2f_tracker="match")), ("lk", dict(f2f_tracker="lk")), ("lk_set", dict(f2f_tracker="lk", lk=LK)),
    ("lk_value", dict(f2f_tracker="lk", lk=_lib.LKOptions(half=5, levels=1))), ("tracker_flow", dict(f2f_tracker="flow")),
    ("lk_alone", dict(lk=LK)), ("lk_half_11", dict(f2f_tracker="lk", lk=dict(half=11))),
    ("lk_unknown", dict(f2f_tracker="lk", lk=dict(window=4))), ("lk_5", dict(f2f_tracker="lk", lk=5)),
    ("slk", dict(stereo_refine="lk")), ("slk_set", dict(stereo_refine="lk", stereo_lk=SLK)),
    ("slk_value", dict(stereo_refine="lk", stereo_lk=_lib.StereoLKOptions(half=2))), ("refine_flow", dict(stereo_refine="flow")),
    ("slk_alone", dict(stereo_lk=SLK)), ("slk_half_11", dict(stereo_refine="lk", stereo_lk=dict(half=11))),
    ("cyclic_false", dict(cyclic_columns=False)),
    # pairs that are refused together
    ("lk+cross_f2f", dict(f2f_tracker="lk", cross_check_f2f=True)), ("lk+gated_f2f", dict(f2f_tracker="lk", lk=LK, gated_f2f=True)),
    ("lk+ratio_f2f", dict(f2f_tracker="lk", ratio_f2f=True, ratio=0.75)),
    ("lk+stereo_side", dict(f2f_tracker="lk", lk=LK, cross_check_stereo=True, gated_stereo=True, ratio_stereo=True, ratio=0.75)),
    # two rules broken at once: which one speaks
    ("lk_alone+slk_alone", dict(lk=LK, stereo_lk=SLK)), ("tracker_flow+refine_flow", dict(f2f_tracker="flow", stereo_refine="flow")),
    ("lk+cross_f2f+refine_flow", dict(f2f_tracker="lk", cross_check_f2f=True, stereo_refine="flow")),
    ("cap_300+lk_alone", dict(gated_f2f=True, gated_max_distance=300, lk=LK)),
    ("ratio_0.7+slk_alone", dict(ratio_stereo=True, ratio=0.7, stereo_lk=SLK)),
    ("subpix_6+ratio_0.7", dict(subpix=6, ratio_f2f=True, ratio=0.7)), ("subpix_6+tracker_flow", dict(subpix=6, f2f_tracker="flow")),
    ("lk_half_11+slk_half_11", dict(f2f_tracker="lk", lk=dict(half=11), stereo_refine="lk", stereo_lk=dict(half=11))),
    ("lk_half_11+cross_f2f", dict(f2f_tracker="lk", lk=dict(half=11), cross_check_f2f=True)),
    ("all_on", dict(cross_check_stereo=True, gated_stereo=True, gated_max_distance=80, ratio_stereo=True, ratio=0.75, subpix=3,
                    f2f_tracker="lk", lk=LK, stereo_refine="lk", stereo_lk=SLK)),
]
OMNI_W = [
    ("cyclic", dict(cyclic_columns=True)), ("cyclic+gated_f2f", dict(cyclic_columns=True, gated_f2f=True, gated_max_distance=64)),
    ("cyclic+lk2", dict(cyclic_columns=True, f2f_tracker="lk", lk=LK)),
    ("cyclic+lk4", dict(cyclic_columns=True, f2f_tracker="lk", lk=dict(half=4, levels=4))),
    ("cyclic+lk_default", dict(cyclic_columns=True, f2f_tracker="lk")),
    ("cyclic+gated+ratio", dict(cyclic_columns=True, gated_f2f=True, ratio_f2f=True, ratio=0.75)),
    ("cyclic+ratio_f2f", dict(cyclic_columns=True, ratio_f2f=True, ratio=0.75)),
    ("cyclic+all_on", dict(cyclic_columns=True, cross_check_stereo=True, gated_stereo=True, ratio_stereo=True, ratio=0.75, subpix=3,
                           f2f_tracker="lk", lk=LK, stereo_refine="lk", stereo_lk=SLK)),
    # two rules broken at once
    ("cyclic+ratio_0.7", dict(cyclic_columns=True, ratio_f2f=True, ratio=0.7)),
    ("cyclic+gated+ratio_0.7", dict(cyclic_columns=True, gated_f2f=True, ratio_f2f=True, ratio=0.7)),
    ("cyclic+lk4+slk_alone", dict(cyclic_columns=True, f2f_tracker="lk", lk=dict(half=4, levels=4), stereo_lk=SLK)),
    ("cyclic+lk_alone", dict(cyclic_columns=True, lk=LK)), ("cyclic+tracker_flow", dict(cyclic_columns=True, f2f_tracker="flow")),
    ("cyclic+lk+gated_f2f", dict(cyclic_columns=True, f2f_tracker="lk", lk=dict(half=4, levels=4), gated_f2f=True)),
    ("cyclic+lk_half_11", dict(cyclic_columns=True, f2f_tracker="lk", lk=dict(half=11))),
    ("cyclic+refine_flow", dict(cyclic_columns=True, stereo_refine="flow")),
    ("cyclic+cap_300", dict(cyclic_columns=True, gated_f2f=True, gated_max_distance=300)),
    ("cyclic+subpix_6", dict(cyclic_columns=True, subpix=6)),
]
# the pair pipeline without a front end: what needs one, alone and two at once
NO_FRONT_END = [
    ("off", {}), ("lk", dict(f2f_tracker="lk")), ("slk", dict(stereo_refine="lk")), ("subpix_3", dict(subpix=3)),
    ("lk+slk", dict(f2f_tracker="lk", stereo_refine="lk")), ("lk+subpix", dict(f2f_tracker="lk", subpix=3)),
    ("slk+tracker_flow", dict(stereo_refine="lk", f2f_tracker="flow")), ("subpix+ratio_0.7", dict(subpix=3, ratio_f2f=True, ratio=0.7)),
    ("lk_half_11", dict(f2f_tracker="lk", lk=dict(half=11))), ("gated+ratio+cross", dict(gated_f2f=True, ratio_f2f=True, ratio=0.75,
                                                                                        cross_check_f2f=True, gated_max_distance=80)),
]
RGBD = [
    ("off", {}), ("cross", dict(cross_check=True)), ("gated_cap", dict(gated_f2f=True, gated_max_distance=64)),
    ("cap_alone", dict(gated_max_distance=64)), ("cap_300", dict(gated_f2f=True, gated_max_distance=300)),
    ("ratio", dict(ratio_f2f=True, ratio=0.75)), ("ratio_missing", dict(ratio_f2f=True)), ("ratio_0.7", dict(ratio=0.7)),
    ("all_on", dict(cross_check=True, gated_f2f=True, gated_max_distance=80, ratio_f2f=True, ratio=0.75)),
]
RGBD_REFUSED = [      # (RGBDPairPipeline does not take these)
    ("match", dict(f2f_tracker="match")), ("lk", dict(f2f_tracker="lk")), ("lk_set", dict(f2f_tracker="lk", lk=LK)),
    ("lk_alone", dict(lk=LK)), ("tracker_flow", dict(f2f_tracker="flow")), ("slk", dict(stereo_refine="lk")),
    ("slk_alone", dict(stereo_lk=SLK)), ("refine_flow", dict(stereo_refine="flow")), ("cyclic", dict(cyclic_columns=True)),
    ("cyclic_false", dict(cyclic_columns=False)),
    ("lk+slk", dict(f2f_tracker="lk", stereo_refine="lk")), ("slk+cyclic", dict(stereo_refine="lk", cyclic_columns=True)),
    ("lk_alone+cyclic", dict(lk=LK, cyclic_columns=True)), ("cyclic+cap_300", dict(cyclic_columns=True, gated_f2f=True, gated_max_distance=300)),
    ("lk+ratio_0.7", dict(f2f_tracker="lk", ratio_f2f=True, ratio=0.7)), ("refine_flow+ratio_missing", dict(stereo_refine="flow", ratio_f2f=True)),
    ("lk_half_11", dict(f2f_tracker="lk", lk=dict(half=11))),
]


# ---- what stands in for the device ---------------------------------------------------------------------------------------------
def _note(v):
    """A call's argument as a short, stable string."""
    if isinstance(v, torch.Tensor):
        return "T%s" % (tuple(v.shape),)
    if isinstance(v, (bool, int, float, str, type(None))):
        return repr(v)
    if isinstance(v, tuple) and not hasattr(v, "_fields") and all(isinstance(x, (bool, int, float, str, type(None))) for x in v):
        return repr(v)
    return type(v).__name__


def _record(name, result=None):
    def call(self, *args, **kwargs):
        c = [a for a in args if isinstance(a, (_lib.BatchCfg, _lib.RgbdBatchCfg))]
        flags = None if not c else c[0].ransac_flags if isinstance(c[0], _lib.BatchCfg) else c[0].flags
        self.calls.append((name, flags) if not kwargs or c else (name, sorted((k, _note(v)) for k, v in kwargs.items())))
        return result(self, *args, **kwargs) if callable(result) else result
    return call


class Recorder(_Rec):
    """The tests' recorder context with the RGB-D entry points and the pair pipelines' stages recorded as well."""

    def __init__(self, device=None, stream=None):
        _Rec.__init__(self)


for _name, _result in (("rgbd_sequence_workspace", 4096), ("rgbd_pair_batch_workspace", 4096), ("rgbd_pair_batch", None),
                       ("rgbd_sequence_front_end", None), ("rgbd_sequence_front_end_slots", None), ("rgbd_sequence_track", None),
                       ("rgbd_sequence_track_seeds", None), ("rgbd_sequence_copy_slot", None), ("rgbd_sequence_copy_slots", None),
                       ("rgbd_sequence_frame_counts", lambda self, cfg_, w, s, first, n, ws: [7] * n),
                       ("match_1nn_two_launch", None), ("match_1nn_slots", None), ("sort_matches", None), ("stereo_assemble", None),
                       ("refine_stereo_lk", None), ("f2f_assemble", None), ("f2f_assemble_tracked", None), ("f2f_assemble_central", None),
                       ("ransac_abs_pose", None), ("refine_abs_pose", None), ("gray_pyramid", "PYR"), ("gray_pyramid_cyclic", "CPYR"),
                       ("track_lk", lambda self, *a, **k: k["out"]), ("unwrap_prepare", "TABLE"), ("set_hint_shared_device", None),
                       ("median_gray", None), ("detect_gft", None), ("describe_orb", None), ("rgbd_assemble", None)):
    setattr(Recorder, _name, _record(_name, _result))


def _front_end(F=4, nmask=3, cap=8, subpix=None):
    z = lambda shape, dt: torch.zeros(shape, dtype=dt)  # noqa: E731
    P = F * nmask
    v = dict(kp_top=z((P, cap, 2), torch.float32), kp_bot=z((P, cap, 2), torch.float32), desc_top=z((P, cap, 32), torch.uint8),
             desc_bot=z((P, cap, 32), torch.uint8), n_top=z((P,), torch.int32), n_bot=z((P,), torch.int32))
    return SimpleNamespace(F=F, kp_cap=cap, model=SimpleNamespace(nmask=nmask), view_arrays=lambda: v, subpix=subpix,
                           gray=z((2 * F, 10, 40), torch.uint8), gray_rows="rows", keep_panoramas=False)


@contextlib.contextmanager
def host_only():
    """torch's device side and the front end replaced by stand-ins (what the tests' host_only fixture does, and the rest that
    OverlappedFramePairs and the multi-sequence engines touch)."""
    ev = SimpleNamespace(record=lambda *a: None, elapsed_time=lambda *a: 0.0)
    built = []

    def image_front_end(ctx, model, nframes, **kw):
        built.append(dict((k, _note(v)) for k, v in sorted(kw.items())))
        return _front_end(F=nframes, subpix=_lib.subpix_half(kw.get("subpix")))
    patches = [(torch.Tensor, "pin_memory", lambda self, *a, **k: self), (torch.cuda, "Event", lambda *a, **k: ev),
               (torch.cuda, "Stream", lambda *a, **k: SimpleNamespace(wait_event=lambda *a: None, synchronize=lambda: None)),
               (torch.cuda, "stream", lambda s: contextlib.nullcontext()), (torch.cuda, "synchronize", lambda *a, **k: None),
               (pipeline, "Context", Recorder), (frontend, "ImageFrontEnd", image_front_end),
               (frontend, "DeviceImageModel", lambda ctx, gums, shape: _model())]
    old = [getattr(o, n) for o, n, _ in patches]
    for o, n, v in patches:
        setattr(o, n, v)
    try:
        yield built
    finally:
        for (o, n, _), v in zip(patches, old):
            setattr(o, n, v)


def _rig(w_top=1200.0, w_bot=None):
    geo = lambda w: (w, 300.0, 0.005, 1.2)  # noqa: E731
    return pipeline.RigConfig(geo(w_top), geo(w_top if w_bot is None else w_bot), (0, 0, 100.0), (0, 0, -100.0), 500.0, 7000.0)


def _cam():
    return pipeline.RGBDCamConfig(fx=500.0, fy=500.0, center_x=8.0, center_y=6.0)


# ---- outcomes ------------------------------------------------------------------------------------------------------------------
def _digest(value):
    """A hash in place of a blob: the file holds what a reader compares by eye, the rest is compared through this."""
    return hashlib.sha1(json.dumps(value, sort_keys=True).encode()).hexdigest()[:12]


def _calls(ctx):
    """The names of the recorded calls, and a hash of what they carried (the flags of their cfg or their keyword arguments;
    the values of the set_*_options calls)."""
    carried = [[c[0], repr(c[1]) if hasattr(c[1], "_fields") else c[1]] for c in ctx.calls]
    return dict(calls=" ".join(c[0] for c in ctx.calls), carried=_digest(carried))


def _values(obj):
    out = {}
    for name in ("opts", "lk", "stereo_lk", "cyclic", "f2f_tracker"):
        for holder in (obj, getattr(obj, "fam", None)):
            if holder is not None and hasattr(holder, name):
                v = getattr(holder, name)
                out[name] = list(v) if hasattr(v, "_fields") else v
                break
    return out


def _cfg_of(c):
    return dict(flags=c.ransac_flags if isinstance(c, _lib.BatchCfg) else c.flags, cfg=hashlib.sha1(bytes(c)).hexdigest()[:12])


def outcome(build, ctx=None):
    """build() -> the outcome's dict; a ValueError / TypeError / NotImplementedError it raises is the outcome."""
    try:
        return build()
    except (ValueError, TypeError, NotImplementedError, AssertionError) as e:
        out = dict(raises="%s: %s" % (type(e).__name__, e))
        if ctx is not None:
            out["asked"] = _calls(ctx)["calls"]
        return out


def _pair_pipeline(kw, rig, front_end):
    ctx = Recorder()

    def build():
        fe = _front_end() if front_end else None
        more = dict(front_end=fe) if front_end else dict(nmask=3, bucket_cap=8)
        p = pipeline.FramePairPipeline(ctx, rig, 2, frame_cap=16, **more, **kw)
        p.stereo()
        p.track()
        search = {k: _note(v) for k, v in sorted(p._f2f_search.items())}
        stereo = {k: _note(v) for k, v in sorted(p._stereo_search.items())}
        tensors = sorted(k for k, v in vars(p).items() if isinstance(v, torch.Tensor))
        return dict(_values(p), **_calls(ctx), cyc=repr(p._cyc), fe_subpix=fe.subpix if fe else None,
                    built=_digest(dict(f2f_search=search, stereo_search=stereo, tensors=tensors)))
    return outcome(build, ctx)


def _overlapped(kw, rig):
    def build():
        with host_only() as built:
            e = pipeline.OverlappedFramePairs(0, None, (12, 16), rig, 3, n_streams=2, kp_cap=8, frame_cap=16, **kw)
            parts = [dict(_values(p.pipe), fe=built[i], fe_subpix=p.fe.subpix, seed=p.pipe.seed, asked=_calls(p.ctx),
                          f2f_search={k: _note(v) for k, v in sorted(p.pipe._f2f_search.items())}, cyc=repr(p.pipe._cyc))
                     for i, p in enumerate(e.parts)]
            return dict(_values(e), **_calls(e.main), part0=_values(e.parts[0].pipe), fe_subpix=e.parts[0].fe.subpix, parts=_digest(parts))
    return outcome(build)


def _pair_batch(kw, rig):
    ctx = Recorder()

    def build():
        b = pipeline.FramePairBatch(ctx, _model(), rig, 2, **SMALL, **kw)
        b.step()
        b.enqueue()
        return dict(_values(b), **_calls(ctx), **_cfg_of(b.cfg))
    return outcome(build, ctx)


def _sequence(kw, rig):
    ctx = Recorder()

    def build():
        with host_only():
            e = pipeline.SequenceEngine(ctx, _model(), rig, window=2, **SMALL, **kw)
            _drive(e)
            return dict(_values(e), **_calls(ctx), **_cfg_of(e.cfg))
    return outcome(build, ctx)


def _drive_lanes(eng, frame):
    a, b = eng.lane(0), eng.lane(1)
    infos = a.push_window([frame] * 2)
    b.push_window([frame])
    a.promote(infos[1]["slot"])
    a.push_window([frame] * 2)
    a.track(a.key_slot, a.last_slot, 3)


def _multi_sequence(kw, rig):
    ctx = Recorder()

    def build():
        with host_only():
            e = pipeline.MultiSequenceEngine(ctx, _model(), rig, lanes=2, window=2, **SMALL, **kw)
            _drive_lanes(e, np.zeros((12, 16, 3), np.uint8))
            return dict(_values(e), **_calls(ctx), **_cfg_of(e.cfg))
    return outcome(build, ctx)


RGBD_SMALL = dict(image_shape=(12, 16), num_of_features=20, kp_cap=32, frame_cap=32)
RGBD_FRAME = (np.zeros((12, 16, 3), np.uint8), np.zeros((12, 16), np.float32))


def _rgbd_pair_pipeline(kw):
    ctx = Recorder()

    def build():
        p = pipeline.RGBDPairPipeline(ctx, _cam(), 2, **RGBD_SMALL, **kw)
        p.step()
        return dict(_values(p), **_calls(ctx), f2f_search={k: _note(v) for k, v in sorted(p._f2f_search.items())})
    return outcome(build, ctx)


def _rgbd_pair_batch(kw):
    ctx = Recorder()

    def build():
        b = pipeline.RGBDPairBatch(ctx, _cam(), 2, **RGBD_SMALL, **kw)
        b.step()
        return dict(_values(b), **_calls(ctx), **_cfg_of(b.cfg))
    return outcome(build, ctx)


def _rgbd_sequence(kw):
    ctx = Recorder()

    def build():
        with host_only():
            e = pipeline.RGBDSequenceEngine(ctx, _cam(), window=2, **RGBD_SMALL, **kw)
            infos = e.push_window([RGBD_FRAME] * 2)
            e.promote(infos[1]["slot"])
            e.push_window([RGBD_FRAME] * 2)
            e.track(e.key_slot, e.last_slot, 3)
            return dict(_values(e), **_calls(ctx), **_cfg_of(e.cfg))
    return outcome(build, ctx)


def _rgbd_multi_sequence(kw):
    ctx = Recorder()

    def build():
        with host_only():
            e = pipeline.RGBDMultiSequenceEngine(ctx, _cam(), lanes=2, window=2, **RGBD_SMALL, **kw)
            _drive_lanes(e, RGBD_FRAME)
            return dict(_values(e), **_calls(ctx), **_cfg_of(e.cfg))
    return outcome(build, ctx)


# ---- batch_cfg / rgbd_batch_cfg --------------------------------------------------------------------------------------------------
CFG_SETTINGS = dict(num_of_features=20, kp_cap=32, frame_cap=64, median_win_size=11, quality=0.01, min_distance=5.0, edge=31, thr=None,
                    max_iter=100, adaptive=False, lm_iter=5, detection_method="GFT")
BATCH_CFG = [(n, kw) for n, kw in OMNI_PLAIN if not {"f2f_tracker", "stereo_refine", "lk", "stereo_lk"} & set(kw)] + [
    ("lk", dict(lk=_lib.LKOptions())), ("stereo_lk", dict(stereo_lk=_lib.StereoLKOptions())), ("cyclic", dict(cyclic_columns=True)),
    ("lk+gated_f2f", dict(lk=_lib.LKOptions(), gated_f2f=True)),      # (the caller's check, not batch_cfg's)
    ("all_on", dict(cross_check_stereo=True, cross_check_f2f=True, gated_stereo=True, gated_f2f=True, gated_max_distance=256,
                    ratio_stereo=True, ratio_f2f=True, ratio=63 / 64.0, subpix=5, lk=_lib.LKOptions(), stereo_lk=_lib.StereoLKOptions(),
                    cyclic_columns=True)),
]


def _batch_cfg(kw, solver):
    return outcome(lambda: _cfg_of(pipeline.batch_cfg(_model(), 6, seed=3, ransac_solver=solver, **CFG_SETTINGS, **kw)))


def _batch_cfg_positional(kw):
    return outcome(lambda: _cfg_of(pipeline.batch_cfg(_model(), 2, 20, 32, 64, 11, 0.01, 5.0, 31, None, 100, False, 0, 5, "GP3P", "GFT",
                                                      *kw.pop("positional", ()), **kw)))


def _rgbd_batch_cfg(kw, algorithm):
    settings = dict(CFG_SETTINGS, image_shape=(12, 16), pose_est_algorithm=algorithm)
    return outcome(lambda: _cfg_of(pipeline.rgbd_batch_cfg(_cam(), 6, seed=1, **settings, **kw)))


# ---- run_VO's engine settings ----------------------------------------------------------------------------------------------------
# a case: the setters run_VO calls, in its order, then _sos_engine_settings; ("fm", which, attribute, value) sets a matcher's
# attribute directly (what no setter does: two caps, two ratios)
SOS_SETTINGS = [
    ("off", []), ("cross", [("set_cross_check", True)]), ("cross_stereo", [("set_cross_check", "stereo")]),
    ("gated_64", [("set_gated_matching", True, 64)]), ("gated_f2f", [("set_gated_matching", "f2f")]),
    ("ratio", [("set_ratio_test", True, 0.75)]), ("ratio_stereo", [("set_ratio_test", "stereo", 0.75)]),
    ("ratio_0.7", [("set_ratio_test", True, 0.7)]), ("subpix", [("set_subpixel_refinement", True, 3)]),
    ("subpix_default", [("set_subpixel_refinement", True, None)]), ("subpix_6", [("set_subpixel_refinement", True, 6)]),
    ("subpix_off", [("set_subpixel_refinement", True, 3), ("set_subpixel_refinement", False)]),
    ("lk", [("set_f2f_tracker", "lk")]), ("lk_set", [("set_f2f_tracker", "lk", LK)]), ("lk_match", [("set_f2f_tracker", "lk"), ("set_f2f_tracker", "match")]),
    ("lk_alone", [("set_f2f_tracker", None, LK)]), ("cross_f2f+lk", [("set_cross_check", "f2f"), ("set_f2f_tracker", "lk")]),
    ("slk", [("set_stereo_refinement", "lk")]), ("slk_set", [("set_stereo_refinement", "lk", SLK)]),
    ("slk_off", [("set_stereo_refinement", "lk"), ("set_stereo_refinement", False)]), ("slk_alone", [("set_stereo_refinement", False, SLK)]),
    ("two_caps", [("set_gated_matching", True, 64), ("fm", "motion", "gated_max_distance", 80)]),
    ("two_ratios", [("set_ratio_test", True, 0.75), ("fm", "motion", "ratio", 0.5)]),
    ("orb", [("set_detection_method", "ORB")]), ("sift", [("set_detection_method", "SIFT")]),
    ("all_on", [("set_cross_check", "stereo"), ("set_gated_matching", "stereo", 80), ("set_ratio_test", "stereo", 0.75),
                ("set_subpixel_refinement", True, 4), ("set_f2f_tracker", "lk", LK), ("set_stereo_refinement", "lk", SLK)]),
]
SOS_SETTINGS_W = [
    ("cyclic", [("set_cyclic_columns", True)]), ("cyclic_off", [("set_cyclic_columns", True), ("set_cyclic_columns", False)]),
    ("cyclic+lk2", [("set_f2f_tracker", "lk", LK), ("set_cyclic_columns", True)]),
    ("cyclic+lk_default", [("set_f2f_tracker", "lk"), ("set_cyclic_columns", True)]),
    ("cyclic+gated", [("set_gated_matching", "f2f", 64), ("set_cyclic_columns", True)]),
    ("cyclic+gated+ratio", [("set_gated_matching", "f2f"), ("set_ratio_test", "f2f", 0.75), ("set_cyclic_columns", True)]),
    ("cyclic+all_on", [("set_cross_check", "stereo"), ("set_gated_matching", "stereo", 80), ("set_ratio_test", "stereo", 0.75),
                       ("set_subpixel_refinement", True, 4), ("set_f2f_tracker", "lk", LK), ("set_stereo_refinement", "lk", SLK),
                       ("set_cyclic_columns", True)]),
]
RGBD_SETTINGS = [
    ("off", []), ("cross", [("set_cross_check", True)]), ("cross_stereo", [("set_cross_check", "stereo")]),
    ("gated_64", [("set_gated_matching", True, 64)]), ("ratio", [("set_ratio_test", "f2f", 0.75)]), ("subpix", [("set_subpixel_refinement", True, 3)]),
    ("subpix_off", [("set_subpixel_refinement", False)]), ("lk", [("set_f2f_tracker", "lk")]), ("match", [("set_f2f_tracker", "match")]),
    ("slk", [("set_stereo_refinement", "lk")]), ("slk_off", [("set_stereo_refinement", False)]), ("cyclic", [("set_cyclic_columns", True)]),
    ("cyclic_off", [("set_cyclic_columns", False)]),
    ("all_on", [("set_cross_check", True), ("set_gated_matching", True, 80), ("set_ratio_test", True, 0.75)]),
]
OPTION_KWARGS = ("cross_check_stereo", "cross_check_f2f", "gated_stereo", "gated_f2f", "gated_max_distance", "ratio_stereo", "ratio_f2f",
                 "ratio", "cross_check", "subpix", "f2f_tracker", "lk", "stereo_refine", "stereo_lk", "cyclic_columns")
_SHARED_MODEL = object()      # (the key holds the device model's id: one model for the sweep, so that equal settings give equal keys)


def _settings(steps, rgbd, widths=(1200, 1200)):
    """-> (outcome, cache key or None)"""
    t = cfg_fakes.tracker(rgbd=rgbd)
    if rgbd:
        cm = cfg_fakes.rgbd_cam()
        first = np.zeros((12, 16, 3), np.uint8)
    else:
        cm = cfg_fakes.Rig()
        cm.model = _SHARED_MODEL
        for m, w in zip((cm.top_model, cm.bot_model), widths):
            m.panorama = SimpleNamespace(cols=w, rows=300, pixel_size=0.01, cyl_height_max=1.0)
        first = np.zeros((480, 640, 3), np.uint8)
    t.camera_model = cm
    key = []

    def build():
        for i, step in enumerate(steps):
            try:
                if step[0] == "fm":
                    setattr(getattr(cm, "feature_matcher_for_" + step[1]), step[2], step[3])
                else:
                    getattr(pet, step[0])(t, *step[1:])
            except ValueError as e:
                raise ValueError("[step %d] %s" % (i, e))
        s = (pet._rgbd_engine_settings if rgbd else pet._sos_engine_settings)(t, cm, first)
        if s is None:
            return dict(settings=None)
        args, kwargs, k = s
        key.append(k)
        hash(k)
        return dict(args=" ".join(type(a).__name__ for a in args), keys=" ".join(sorted(kwargs)),
                    options={n: list(kwargs[n]) if hasattr(kwargs[n], "_fields") else kwargs[n] for n in OPTION_KWARGS if n in kwargs},
                    widths=None if rgbd else [args[1].pano_top[0], args[1].pano_bot[0]])
    out = outcome(build)
    return out, key[0] if key else None


# ---- the sweep -------------------------------------------------------------------------------------------------------------------
def _omni_cases():
    """(name, kwargs, rig) of the omnistereo constructors' grid."""
    for name, kw in OMNI_PLAIN:
        yield name, kw, _rig()
    for name, kw in OMNI_W:
        for w in WIDTHS:
            yield "%s@%g" % (name, w), kw, _rig(w)
    # one search serves both views: their widths must agree under the gate
    for name, kw in (("cyclic", dict(cyclic_columns=True)), ("cyclic+gated_f2f", dict(cyclic_columns=True, gated_f2f=True)),
                     ("cyclic+lk2", dict(cyclic_columns=True, f2f_tracker="lk", lk=LK))):
        yield "%s@1200/1208" % name, kw, _rig(1200.0, 1208.0)
        yield "%s@1200/1204" % name, kw, _rig(1200.0, 1204.0)


def record():
    """-> {case id: outcome}"""
    out = {}
    for name, kw, rig in _omni_cases():
        for cls, run in (("FramePairPipeline", lambda kw, rig: _pair_pipeline(kw, rig, True)), ("OverlappedFramePairs", _overlapped),
                         ("FramePairBatch", _pair_batch), ("SequenceEngine", _sequence), ("MultiSequenceEngine", _multi_sequence)):
            out["%s/%s" % (cls, name)] = run(dict(kw), rig)
    for name, kw in NO_FRONT_END:
        out["FramePairPipeline/no_front_end/%s" % name] = _pair_pipeline(dict(kw), _rig(), False)
    for name, kw in OMNI_W[:6]:
        out["FramePairPipeline/no_front_end/%s@1204" % name] = _pair_pipeline(dict(kw), _rig(1204.0), False)
    for name, kw in RGBD:
        out["RGBDPairPipeline/%s" % name] = _rgbd_pair_pipeline(dict(kw))
    out["RGBDPairPipeline/lk"] = _rgbd_pair_pipeline(dict(f2f_tracker="lk"))      # (a TypeError: not its parameter)
    for name, kw in RGBD + RGBD_REFUSED:
        for cls, run in (("RGBDPairBatch", _rgbd_pair_batch), ("RGBDSequenceEngine", _rgbd_sequence),
                         ("RGBDMultiSequenceEngine", _rgbd_multi_sequence)):
            out["%s/%s" % (cls, name)] = run(dict(kw))
    for name, kw in BATCH_CFG:
        out["batch_cfg/GP3P/%s" % name] = _batch_cfg(dict(kw), "GP3P")
    for name, kw in BATCH_CFG[:1] + BATCH_CFG[-2:]:
        out["batch_cfg/P3P/%s" % name] = _batch_cfg(dict(kw), "P3P")
    for name, kw in (("none", {}), ("cross", dict(positional=(True, True))), ("subpix_keyword", dict(subpix=4)),
                     ("up_to_ratio", dict(positional=(False, False, True, True, 80, True, False, 0.75))),
                     ("up_to_subpix", dict(positional=(False, False, False, False, None, False, False, None, 3)))):
        out["batch_cfg/positional/%s" % name] = _batch_cfg_positional(dict(kw))
    for name, kw in RGBD:
        for algorithm in ("EPNP", "GAO") + (("DLS",) if name in ("off", "ratio_0.7") else ()):
            out["rgbd_batch_cfg/%s/%s" % (algorithm, name)] = _rgbd_batch_cfg(dict(kw), algorithm)
    # the engine settings, and which of their cache keys compare equal (the id of the first case with an equal key)
    keyed = []
    cases = [("sos/" + n, s, False, (1200, 1200)) for n, s in SOS_SETTINGS]
    cases += [("sos/%s@%g" % (n, w), s, False, (w, w)) for n, s in SOS_SETTINGS_W for w in (1200, 1204, 1200.5)]
    cases += [("sos/%s@1200/1208" % n, s, False, (1200, 1208)) for n, s in SOS_SETTINGS_W[:1] + SOS_SETTINGS_W[4:5]]
    cases += [("sos/off_again", [], False, (1200, 1200)), ("sos/lk_set_again", [("set_f2f_tracker", "lk", dict(LK))], False, (1200, 1200))]
    cases += [("rgbd/" + n, s, True, None) for n, s in RGBD_SETTINGS] + [("rgbd/off_again", [], True, None)]
    for name, steps, rgbd, widths in cases:
        o, key = _settings(steps, rgbd, widths)
        if key is not None:
            same = [n for n, k in keyed if k == key]
            if same and hash(key) != hash(dict(keyed)[same[0]]):
                o["hash_differs"] = True
            o["key_of"] = same[0] if same else name
            keyed.append((name, key))
        out["engine_settings/%s" % name] = o
    return out


def main(argv):
    if len(argv) != 2:
        sys.exit(__doc__)
    out = record()
    with open(argv[1], "w") as f:      # one case per line
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(out[k], sort_keys=True)) for k in sorted(out)) + "\n}\n")
    print("%d cases, %d of them refusals -> %s" % (len(out), sum("raises" in o for o in out.values()), argv[1]))


if __name__ == "__main__":
    main(sys.argv)
