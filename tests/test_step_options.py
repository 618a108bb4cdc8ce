"""CPU: what the Python layers do with the step options is what they did before the options became one value
(_lib.StepOptions).  scripts/record_step_options.py sweeps the public constructors of pipeline.py, batch_cfg / rgbd_batch_cfg
and run_VO's engine settings over a grid of option settings -- every option off and on, every pair that is refused together,
settings that break two rules at once (so the ORDER of the checks is compared), panoramas 1200, 1204 and 1200.5 columns wide
-- and writes one outcome per case: the exception, or the flags word, a hash of the cfg's bytes, the recorded device calls and
the values of .opts / .lk / .stereo_lk / .cyclic.  tests/golden/step_options_parent.json holds the outcomes of the commit
before the refactor, written by that script from that commit's tree; here every case is computed again and compared."""
import importlib.util
import json
import os

import pytest

from vo_single_camera_sos_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "step_options_parent.json")))
GROUPS = sorted({k.split("/")[0] for k in GOLDEN})


@pytest.fixture(scope="module")
def outcomes():
    spec = importlib.util.spec_from_file_location("record_step_options", os.path.join(ROOT, "scripts", "record_step_options.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return json.loads(json.dumps(mod.record()))      # (as the file holds them: tuples are lists)


def test_the_sweep_is_the_recorded_one(outcomes):
    assert sorted(outcomes) == sorted(GOLDEN) and len(GOLDEN) > 700
    assert {"FramePairPipeline", "OverlappedFramePairs", "FramePairBatch", "SequenceEngine", "MultiSequenceEngine", "RGBDPairPipeline",
            "RGBDPairBatch", "RGBDSequenceEngine", "RGBDMultiSequenceEngine", "batch_cfg", "rgbd_batch_cfg", "engine_settings"} == set(GROUPS)
    refusals = [k for k, o in GOLDEN.items() if "raises" in o]
    assert 400 < len(refusals) < len(GOLDEN) - 250
    assert all(o.get("asked", "") == "" for o in GOLDEN.values())      # every refusal came before the first device call


@pytest.mark.parametrize("group", GROUPS)
def test_every_case_is_what_the_parent_commit_gave(outcomes, group):
    differ = {k: (outcomes[k], GOLDEN[k]) for k in GOLDEN if k.startswith(group + "/") and outcomes[k] != GOLDEN[k]}
    assert not differ, "%d cases differ, the first: %s" % (len(differ), sorted(differ.items())[0])


def test_step_options_is_one_hashable_value_and_the_only_place_that_ors_the_flags():
    o = _lib.StepOptions()
    assert o == (_lib.MatchOptions(), None, None, None, False) and o.flags() == 0 and hash(o) == hash(_lib.StepOptions())
    lk, slk = _lib.LKOptions(half=4), _lib.StereoLKOptions(half=3)
    m = _lib.MatchOptions(cross_check_stereo=True, gated_stereo=True, gated_max_distance=80, ratio_stereo=True, ratio=0.75)
    on = _lib.StepOptions(m, 3, lk, slk, True)
    assert on.flags() == m.flags() | _lib.subpix_flags(3) | _lib.FLAG_LK_F2F | _lib.FLAG_LK_STEREO | _lib.FLAG_CYCLIC_F2F
    for field, bit in (("lk", _lib.FLAG_LK_F2F), ("stereo_lk", _lib.FLAG_LK_STEREO), ("cyclic", _lib.FLAG_CYCLIC_F2F)):
        assert on._replace(**{field: None if field != "cyclic" else False}).flags() == on.flags() & ~bit
    assert on._replace(subpix=None).flags() == on.flags() & ~(_lib.FLAG_SUBPIX | _lib.SUBPIX_HALF_MASK)
    assert len({on, on._replace(cyclic=False), on._replace(lk=_lib.LKOptions(half=5)), _lib.StepOptions(m, 3, lk, slk, True)}) == 3
    # the keyword form and back: the four later options are left out when they are off
    assert o.kwargs() == dict(_lib.MatchOptions()._asdict(), subpix=None)
    kw = on.kwargs()
    assert kw == dict(m._asdict(), subpix=3, f2f_tracker="lk", lk=lk, stereo_refine="lk", stereo_lk=slk, cyclic_columns=True)
    assert _lib.StepOptions.of(rig=(1200, 1200), **kw) == on
    assert _lib.StepOptions.rgbd(**m._replace(cross_check_stereo=False, gated_stereo=False, ratio_stereo=False).rgbd_kwargs()).match == \
        _lib.MatchOptions.rgbd(gated_max_distance=80, ratio=0.75)
