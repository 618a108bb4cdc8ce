"""GPU: sosvo_refine_stereo_lk against tests/refstereolk.py bit for bit -- 2 frames, 3 masks, cap 16, 96 x 128 images, bottom
counts (16, 1, 0, 7, 16, 3); windows on a 16-lane group (half 2, 4) and on a whole wave (half 10); with and without a row
range; dropped and out-of-range keys, non-finite keypoints, max_shift 0.25, eps 0; the sentinel fill of everything the stage
is handed and must not write (it never sees the descriptors); the composition Context.track_lk + acceptance; the pre-gate against refining everything; the planted-shift
bound of tests/test_stereo_lk_reference.py on the device; the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import reflk
import refstereolk as ref
from vo_single_camera_sos_amd import _lib
from vo_single_camera_sos_amd.device import SosvoError

pytestmark = pytest.mark.gpu

F, NM, CAP, ROWS, COLS = 2, 3, 16, 96, 128
N_BOT = (16, 1, 0, 7, 16, 3)
N_TOP = (16, 5, 3, 9, 12, 4)
SHIFTS = (ref.SHIFTS[0], ref.SHIFTS[2])          # frame 0, frame 1
SENTINEL = np.float32(-123.25)
ROW_RANGE = np.array([[36, 62], [9, 57]], np.int32)         # (top view, bottom view): windows are clamped, centres fall outside


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


@pytest.fixture(scope="module")
def scene():
    """Host arrays, built once and never written: two frames (top = a texture, bottom = the texture shifted), top keypoints on
    and off the pixel grid, bottom keypoints = the true partner rounded, some 1 px further; rows beyond the counts hold the
    sentinel."""
    rng = np.random.default_rng(41)
    gray = np.stack([reflk.texture(7, ROWS, COLS), reflk.texture(9, ROWS, COLS),
                     reflk.texture(7, ROWS, COLS, SHIFTS[0]), reflk.texture(9, ROWS, COLS, SHIFTS[1])])
    P = F * NM
    kp_top = np.full((P, CAP, 2), SENTINEL, np.float32)
    kp_bot = np.full((P, CAP, 2), SENTINEL, np.float32)
    keys = np.full((P, CAP), 0x12345678, np.uint32)          # (rows beyond n_bot: never read)
    for p in range(P):
        sh = np.asarray(SHIFTS[p // NM])
        for t in range(N_TOP[p]):
            xy = rng.uniform((24, 30), (COLS - 24, ROWS - 30))
            kp_top[p, t] = np.rint(xy) if t % 2 else xy
        for q in range(N_BOT[p]):
            t = int(rng.integers(0, N_TOP[p]))
            kp_bot[p, q] = np.rint(kp_top[p, t].astype(np.float64) + sh) + ((1.0, -1.0) if q % 3 == 2 else (0.0, 0.0))
            keys[p, q] = np.uint32(t | (int(rng.integers(0, 90)) << 20))
    return dict(gray=gray, kp_top=kp_top, kp_bot=kp_bot, keys=keys, n_top=np.array(N_TOP, np.int32), n_bot=np.array(N_BOT, np.int32))


def _device(ctx, s, kp_top=None, kp_bot=None, keys=None, row_range=None, min_disp=-1.0, max_hdiff=0.0, **opts):
    """-> (kp_bot, status, kp_top, n_top, n_bot, keys) as numpy after the stage; the status buffer starts as 0xA5."""
    t = dict(kp_top=_dev(ctx, s["kp_top"] if kp_top is None else kp_top), kp_bot=_dev(ctx, s["kp_bot"] if kp_bot is None else kp_bot),
             keys=_dev(ctx, s["keys"] if keys is None else keys), n_top=_dev(ctx, s["n_top"]), n_bot=_dev(ctx, s["n_bot"]))
    status = torch.full((F * NM, CAP), 0xA5, dtype=torch.uint8, device=ctx.device)
    ctx.refine_stereo_lk(_dev(ctx, s["gray"]), t["kp_top"], t["n_top"], t["kp_bot"], t["n_bot"], t["keys"], NM, min_disp, max_hdiff,
                         stereo_lk=opts, row_range=None if row_range is None else _dev(ctx, row_range), status=status)
    ctx.synchronize()
    return (t["kp_bot"].cpu().numpy(), status.cpu().numpy()) + tuple(t[k].cpu().numpy() for k in ("kp_top", "n_top", "n_bot", "keys"))


def _reference(s, kp_top=None, kp_bot=None, keys=None, row_range=None, min_disp=-1.0, max_hdiff=0.0, pre_gate=True, **opts):
    return ref.refine(s["gray"], NM, s["kp_top"] if kp_top is None else kp_top, s["n_top"], s["kp_bot"] if kp_bot is None else kp_bot,
                      s["n_bot"], s["keys"] if keys is None else keys, row_range=row_range, min_disp=min_disp, max_hdiff=max_hdiff,
                      pre_gate=pre_gate, status=np.full((F * NM, CAP), 0xA5, np.uint8), **dict(ref.DEFAULTS, **opts))


def _assert_equal(got, want, what):
    for g, w, name in ((_u32(got[0]), _u32(want[0]), "kp_bot"), (got[1], want[1], "status")):
        bad = np.argwhere(g != w)
        assert bad.size == 0, (what, name, bad[:4], [(g[tuple(b)], w[tuple(b)]) for b in bad[:4]])


@pytest.mark.parametrize("half", [2, 4, 10])
@pytest.mark.parametrize("rows", [None, ROW_RANGE], ids=["all_rows", "row_range"])
def test_stage_equals_the_reference(ctx, scene, half, rows):
    got = _device(ctx, scene, row_range=rows, half=half)
    want = _reference(scene, row_range=rows, half=half)
    _assert_equal(got, want, (half, rows is not None))
    if rows is None:                                         # the stage does something
        assert want[1][0, :16].sum() >= 12 and want[1][4, :16].sum() >= 12
    else:                                                    # ... and the range loses the top keypoints outside it
        assert 0 < (want[1] == 1).sum() < (_reference(scene, half=half)[1] == 1).sum()
    # what the stage must not write: rows at and beyond n_bot (sentinels), kp_top, the counts, the keys
    for p, n in enumerate(N_BOT):
        assert (got[0][p, n:] == SENTINEL).all() and (got[1][p, n:] == 0xA5).all(), p
    assert np.array_equal(_u32(got[2]), _u32(scene["kp_top"])) and np.array_equal(got[5], scene["keys"])
    assert np.array_equal(got[3], scene["n_top"]) and np.array_equal(got[4], scene["n_bot"])


def test_dropped_keys_bad_indices_and_non_finite_keypoints(ctx, scene):
    keys, kb, kt = scene["keys"].copy(), scene["kp_bot"].copy(), scene["kp_top"].copy()
    keys[0, 2] = ref.KEY_NONE
    keys[0, 3] = np.uint32(N_TOP[0] | (5 << 20))             # a train index at n_top ...
    keys[3, 1] = np.uint32(N_TOP[3] | (5 << 20))
    keys[4, 0] = np.uint32(0xFFFFF)                          # ... and far beyond the table
    keys[1, 0] = ref.KEY_NONE                                # a problem left with nothing to track
    kb[0, 5, 0] = np.nan
    kb[0, 6, 1] = np.inf
    kb[4, 9] = (-np.inf, np.nan)
    kt[3, :, 0] = np.where(np.arange(CAP) % 2 == 0, np.nan, kt[3, :, 0])
    for half in (4, 10):
        got = _device(ctx, scene, kp_top=kt, kp_bot=kb, keys=keys, half=half)
        want = _reference(scene, kp_top=kt, kp_bot=kb, keys=keys, half=half)
        _assert_equal(got, want, half)
        for p, q in ((0, 2), (0, 3), (3, 1), (4, 0), (1, 0), (0, 5), (0, 6), (4, 9)):
            assert got[1][p, q] == 0 and np.array_equal(_u32(got[0][p, q]), _u32(kb[p, q])), (p, q)
        assert got[1][0, :16].sum() >= 8


@pytest.mark.parametrize("opts", [dict(max_shift=0.25), dict(eps=0.0), dict(eps=0.0, max_iter=3, half=3), dict(max_shift=1.5, min_eig=0.0)],
                         ids=["max_shift_0.25", "eps_0", "eps_0_3_iterations", "max_shift_1.5_min_eig_0"])
def test_settings(ctx, scene, opts):
    got, want = _device(ctx, scene, **opts), _reference(scene, **opts)
    _assert_equal(got, want, opts)
    if opts.get("max_shift") == 0.25:                        # the rows 1 px off revert; some partner lies within a quarter pixel
        assert not want[1][0, 2:16:3].any() and want[1].any()
        assert np.abs(want[0][want[1] == 1] - scene["kp_bot"][want[1] == 1]).max() <= 0.25


def test_pre_gate_equals_the_reference_and_never_changes_what_passes(ctx, scene):
    """The rig's gates (2.5 px, 1 px): frame 0 (disparity 7.21) passes, frame 1 (disparity 1.3, 1 px guesses at 0) straddles
    the gate; bottom keypoints pushed beyond the loosened bounds are skipped."""
    kb = scene["kp_bot"].copy()
    kb[0, 0, 0] += 7.0                                       # |du| about 7 > 2.5 + 4
    kb[4, 1, 1] += 5.0                                       # dv about 1.3 - 5 < 1 - 4
    kb[4, 2, 0] -= 6.0                                       # |du| about 6 <= 6.5: tracked
    with_gate = _device(ctx, scene, kp_bot=kb, min_disp=1.0, max_hdiff=2.5)
    want = _reference(scene, kp_bot=kb, min_disp=1.0, max_hdiff=2.5)
    _assert_equal(with_gate, want, "pre-gate")
    assert with_gate[1][0, 0] == 0 and with_gate[1][4, 1] == 0
    everything = _device(ctx, scene, kp_bot=kb)              # both gates disabled: no pre-gate
    _assert_equal(everything, _reference(scene, kp_bot=kb, pre_gate=False), "no pre-gate")
    t_of = scene["keys"] & ref.KEY_IDX_MASK
    n = 0
    for p in range(F * NM):
        for q in range(N_BOT[p]):
            a, b = everything[0][p, q], with_gate[0][p, q]
            ok = [ref.passes_gates(*scene["kp_top"][p, t_of[p, q]], *x, 1.0, 2.5) for x in (a, b)]
            assert ok[0] == ok[1], (p, q)
            if ok[0]:
                n += 1
                assert np.array_equal(_u32(a), _u32(b)) and everything[1][p, q] == with_gate[1][p, q], (p, q)
    assert n >= 20


def test_stage_is_track_lk_plus_acceptance(ctx, scene):
    """The same tables through Context.track_lk (one level, the initial-flow flag: problem p tracks from image p // NM to image
    F + p // NM; a bottom keypoint's start is its partner) and the acceptance rule on the host."""
    s = scene
    P = F * NM
    t_of = (s["keys"] & ref.KEY_IDX_MASK).astype(np.int64)
    prev = np.zeros((P, CAP, 2), np.float32)
    for p in range(P):
        prev[p, :N_BOT[p]] = s["kp_top"][p, t_of[p, :N_BOT[p]]]
    for half in (4, 10):
        pyr = ctx.gray_pyramid(_dev(ctx, s["gray"]), 1)
        img = np.arange(P, dtype=np.int32) // NM
        nxt = _dev(ctx, s["kp_bot"])
        res = ctx.track_lk(pyr, _dev(ctx, img), _dev(ctx, img + F), _dev(ctx, prev), _dev(ctx, s["n_bot"]), half=half, next_pts=nxt)
        ctx.synchronize()
        nx, st = res[0].cpu().numpy(), res[1].cpu().numpy()
        want_kp, want_st = s["kp_bot"].copy(), np.full((P, CAP), 0xA5, np.uint8)
        for p in range(P):
            for q in range(N_BOT[p]):
                d = nx[p, q].astype(np.float64) - s["kp_bot"][p, q].astype(np.float64)
                ok = st[p, q] == 1 and abs(d[0]) <= half and abs(d[1]) <= half
                want_st[p, q] = 1 if ok else 0
                if ok:
                    want_kp[p, q] = nx[p, q]
        _assert_equal(_device(ctx, s, half=half), (want_kp, want_st), half)


@pytest.mark.parametrize("k", range(3))
def test_planted_shifts_on_the_device(ctx, k):
    """The bound of test_planted_shifts_are_recovered, on the device: every track accepted, the largest error below twice the
    CPU reference's figure (0.0653 / 0.0716 / 0.0719 px at half 4)."""
    t = ref.planted_tables(ref.SHIFTS[k])
    kp_bot = _dev(ctx, t["kp_bot"])
    _, st = ctx.refine_stereo_lk(_dev(ctx, t["gray"]), _dev(ctx, t["kp_top"]), _dev(ctx, t["n_top"]), kp_bot, _dev(ctx, t["n_bot"]),
                                 _dev(ctx, t["keys"]), 1)
    ctx.synchronize()
    err = ref.errors(kp_bot.cpu().numpy(), t["truth"])
    print("shift %r: mean %.4f max %.4f px" % (ref.SHIFTS[k], err.mean(), err.max()))
    assert st.cpu().numpy()[0, :120].all()
    assert err.max() < 2.0 * ref.MEASURED_MAX[4][k]


def test_refusals(ctx, scene):
    s = scene
    lib, h = _lib.load(), ctx._h
    d = {k: _dev(ctx, s[k]) for k in ("gray", "kp_top", "kp_bot", "keys", "n_top", "n_bot")}
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(nimg=2 * F, rows=ROWS, cols=COLS, nmask=NM, cap=CAP, opt=None, gray=True, keys=True, min_disp=-1.0, max_hdiff=0.0):
        o = _lib.StereoLkOptionsStruct.of(_lib.StereoLKOptions())
        for k, v in (opt or {}).items():
            setattr(o, k, v)
        return lib.sosvo_refine_stereo_lk(h, p(d["gray"]) if gray else None, nimg, rows, cols, None, nmask, cap, p(d["kp_top"]),
                                          p(d["n_top"]), p(d["kp_bot"]), p(d["n_bot"]), p(d["keys"]) if keys else None, min_disp,
                                          max_hdiff, ctypes.byref(o), None)
    assert call() == 0                                       # (status is optional)
    for bad in (dict(nimg=3), dict(nimg=-2), dict(rows=0), dict(cols=16385), dict(nmask=0), dict(cap=0), dict(cap=4097), dict(gray=False),
                dict(keys=False), dict(min_disp=float("nan")), dict(max_hdiff=float("nan")), dict(nimg=2 * 32768, nmask=1)):
        assert call(**bad) == -1, bad
    for bad in (dict(half=1), dict(half=11), dict(max_iter=0), dict(max_iter=31), dict(eps=-1.0), dict(eps=float("nan")),
                dict(eps=float("inf")), dict(min_eig=-1e-9), dict(min_eig=float("inf")), dict(max_shift=-0.5),
                dict(max_shift=float("nan")), dict(max_shift=float("inf"))):
        assert call(opt=bad) == -1, bad
        o = _lib.StereoLkOptionsStruct.of(_lib.StereoLKOptions())
        for k, v in bad.items():
            setattr(o, k, v)
        assert lib.sosvo_set_stereo_lk_options(h, ctypes.byref(o)) == -1, bad
    assert lib.sosvo_set_stereo_lk_options(h, None) == -1
    ctx.synchronize()
    # the context's settings are what a NULL options pointer means: half 10 there, half 10 explicitly
    ctx.set_stereo_lk_options(dict(half=10, max_shift=2.0))
    kb = _dev(ctx, s["kp_bot"])
    assert lib.sosvo_refine_stereo_lk(h, p(d["gray"]), 2 * F, ROWS, COLS, None, NM, CAP, p(d["kp_top"]), p(d["n_top"]), p(kb), p(d["n_bot"]),
                                      p(d["keys"]), -1.0, 0.0, None, None) == 0
    ctx.synchronize()
    assert np.array_equal(_u32(kb.cpu().numpy()), _u32(_reference(s, half=10, max_shift=2.0)[0]))
    ctx.set_stereo_lk_options(None)
    assert ctx.stereo_lk_options == _lib.StereoLKOptions()
    with pytest.raises(SosvoError):
        ctx.refine_stereo_lk(d["gray"][:3], d["kp_top"], d["n_top"], d["kp_bot"], d["n_bot"], d["keys"], NM)
    with pytest.raises(ValueError):
        ctx.refine_stereo_lk(d["gray"], d["kp_top"], d["n_top"], d["kp_bot"], d["n_bot"], d["keys"], NM, stereo_lk=dict(half=11))
