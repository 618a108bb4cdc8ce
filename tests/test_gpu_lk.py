"""GPU: pyramidal Lucas-Kanade tracking -- sosvo_gray_pyramid and sosvo_track_lk against tests/reflk.py bit for bit (1 and 3
levels; windows on a 16-lane group and on a whole wave; counts 0, 1, a full wave, more than one; integer, fractional, corner,
outside and NaN starts; eps 0; the initial-flow flag; a row range; the forward-backward check; the image indirection), the
planted shifts of tests/test_lk_reference.py on the device within the bounds derived there, the argument refusals,
sosvo_f2f_assemble_tracked against a numpy restatement, FramePairPipeline(f2f_tracker="lk") on two rendered pairs beside the
matcher (figures printed, one sanity bound), and the host mirror common_cv.calc_optical_flow_pyr_lk."""
import ctypes

import numpy as np
import pytest
import torch

import matching_scenes as scenes
import reflk
import synth
from test_lk_reference import LARGE_SHIFT, RECOVERED_LARGE, RECOVERED_SMALL, SMALL_SHIFT
from vo_single_camera_sos_amd import _lib, synthetic
from vo_single_camera_sos_amd.device import make_rig
from vo_single_camera_sos_amd.frontend import DeviceImageModel, ImageFrontEnd
from vo_single_camera_sos_amd.omnistereo import common_cv
from vo_single_camera_sos_amd.pipeline import FramePairPipeline, RigConfig

pytestmark = pytest.mark.gpu

NIMG, ROWS, COLS, CAP, MAX_ITER = 4, 96, 128, 80, 10
COUNTS = (80, 1, 64, 0)           # more than one wave of groups, a lone point, full waves, nothing
FEW = (12, 1, 12, 0)               # what the whole-wave window (half 10) is compared on: the reference is slow there
PREV_IMG, NEXT_IMG = (0, 2, 0, 2), (1, 3, 1, 3)    # images view-major: pair A = images (0, 1) of view 0, pair B = (2, 3) of view 1
SENTINEL = np.float32(-123.25)
ROW_RANGE = np.array([[21, 70], [9, 96]], np.int32)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _starts(rng, count, other):
    """count starts: integer and fractional ones inside the image, anywhere in the image and a little outside, and in the
    first rows the image corners, a point just outside and a NaN."""
    kp = np.full((CAP, 2), SENTINEL, np.float32)
    for k in range(count):
        kind = k % 3
        if kind == 0:
            kp[k] = rng.integers(14, COLS - 14), rng.integers(26, ROWS - 30)
        elif kind == 1:
            kp[k] = rng.uniform(14, COLS - 14), rng.uniform(26, ROWS - 30)
        else:
            kp[k] = rng.uniform(-2, COLS + 1), rng.uniform(-2, ROWS + 1)
    if count >= 6:
        kp[2] = 0, 0
        kp[3] = COLS - 1, ROWS - 1
        kp[4] = (np.nan, 20) if other else (20, np.inf)
        kp[5] = COLS - 0.4, -0.6                            # just outside: rounds to a centre off the image
    return kp


@pytest.fixture(scope="module")
def scene():
    """Four images (two shifted pairs), one set of starts, and the reference pyramids per (levels, row range): host arrays,
    built once and never written."""
    rng = np.random.default_rng(23)
    gray = np.stack([reflk.texture(11, ROWS, COLS), reflk.texture(11, ROWS, COLS, (1.37, -0.71)),
                     reflk.texture(12, ROWS, COLS), reflk.texture(12, ROWS, COLS, LARGE_SHIFT)])
    pts = np.stack([_starts(rng, c, p & 1) for p, c in enumerate(COUNTS)])
    s = dict(gray=gray, pts=pts, n=np.array(COUNTS, np.int32), few=np.array(FEW, np.int32), pyrs={})

    def pyrs(levels, row_range=None):
        key = (levels, None if row_range is None else row_range.tobytes())
        if key not in s["pyrs"]:
            s["pyrs"][key] = reflk.pyramid_set(gray, levels, row_range)
        return s["pyrs"][key]
    s["ref_pyrs"] = pyrs
    return s


def _device_track(ctx, gray, levels, pts, n, half, max_iter=MAX_ITER, eps=0.01, min_eig=1e-4, guess=None, fb_max=None,
                  row_range=None, prev_img=PREV_IMG, next_img=NEXT_IMG):
    """-> (next, status, err[, back]) as numpy; every output buffer starts as the sentinel (0xA5 for the status)."""
    rr = None if row_range is None else _dev(ctx, row_range)
    pyr = ctx.gray_pyramid(_dev(ctx, gray), levels, row_range=rr)
    P = len(prev_img)
    nxt = torch.full((P, CAP, 2), float(SENTINEL), dtype=torch.float32, device=ctx.device)
    out = (nxt, torch.full((P, CAP), 0xA5, dtype=torch.uint8, device=ctx.device),
           torch.full((P, CAP), float(SENTINEL), dtype=torch.float32, device=ctx.device),
           torch.full((P, CAP, 2), float(SENTINEL), dtype=torch.float32, device=ctx.device))
    if guess is not None:
        nxt.copy_(_dev(ctx, guess))
    res = ctx.track_lk(pyr, _dev(ctx, np.array(prev_img, np.int32)), _dev(ctx, np.array(next_img, np.int32)), _dev(ctx, pts),
                       _dev(ctx, n), half=half, max_iter=max_iter, eps=eps, min_eig=min_eig,
                       next_pts=nxt if guess is not None else None, fb_max=fb_max, out=out)
    ctx.synchronize()
    return tuple(t.cpu().numpy() for t in res)


def _sentinels(guess=None):
    P = len(PREV_IMG)
    return (np.full((P, CAP, 2), SENTINEL, np.float32) if guess is None else guess.copy(), np.full((P, CAP), 0xA5, np.uint8),
            np.full((P, CAP), SENTINEL, np.float32), np.full((P, CAP, 2), SENTINEL, np.float32))


def _assert_equal(got, want, n, what):
    """next / err / back as uint32 bit patterns, status as bytes; the rows at and beyond n[p] hold what they held."""
    assert len(got) == len(want)
    for g, w, name in zip(got, want, ("next", "status", "err", "back")):
        g, w = (a if a.dtype == np.uint8 else _u32(a) for a in (g, w))
        bad = np.argwhere(g != w)
        assert bad.size == 0, (what, name, bad[:4], [(g[tuple(b)], w[tuple(b)]) for b in bad[:4]])
    assert sum(int(c) for c in n) > 0


def _reference(s, levels, n, half, row_range=None, guess=None, fb_max=None, **kw):
    return reflk.track_problems(s["ref_pyrs"](levels, row_range), PREV_IMG, NEXT_IMG, s["pts"], n, half, next_pts=guess,
                                fb_max=fb_max, out=_sentinels(guess), **kw)


# ---- the pyramid -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,row_range", [(ROWS, COLS, None), (ROWS, COLS, ROW_RANGE), (95, 127, None),
                                                 (95, 127, np.array([[94, 95], [-3, 40]], np.int32))])
def test_pyramid_equals_the_reference_byte_for_byte(ctx, rows, cols, row_range):
    """4 levels; the device buffer starts as 0xAB, so the rows outside a range are seen to stay."""
    rng = np.random.default_rng(rows)
    gray = rng.integers(0, 256, (NIMG, rows, cols), dtype=np.uint8)
    nbytes = _lib.gray_pyramid_bytes(NIMG, rows, cols, 4)
    sizes = reflk.level_sizes(rows, cols, 4)
    assert nbytes == NIMG * sum(r * c for r, c in sizes[1:])
    d_gray = _dev(ctx, gray)
    pyr = ctx.gray_pyramid(d_gray, 4, row_range=None if row_range is None else _dev(ctx, row_range))
    pyr.upper.fill_(0xAB)
    pyr = ctx.gray_pyramid(d_gray, 4, row_range=pyr.row_range, out=pyr)
    ctx.synchronize()
    for i in range(NIMG):
        fill = [np.full(sz, 0xAB, np.uint8) for sz in sizes[1:]]
        want, _ = reflk.pyramid(gray[i], 4, None if row_range is None else row_range[i // 2], fill=fill)
        for l in range(1, 4):
            assert np.array_equal(pyr.level(l)[i].cpu().numpy(), want[l]), (i, l)
    assert np.array_equal(d_gray.cpu().numpy(), gray)


# ---- the tracker against the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("half", [2, 4, 10])
def test_track_equals_the_reference_bit_for_bit(ctx, scene, half, levels):
    s = scene
    n = s["few"] if half == 10 else s["n"]
    got = _device_track(ctx, s["gray"], levels, s["pts"], n, half)
    _assert_equal(got, _reference(s, levels, n, half, max_iter=MAX_ITER), n, (half, levels))
    nxt, st, err = got
    assert st[0, 4] == 0 and np.array_equal(_u32(nxt[0, 4]), _u32(s["pts"][0, 4]))       # the non-finite start: next = prev
    assert st[0, 5] == 0                                                                 # the start off the image
    tracked = st[0, :n[0]] == 1
    assert tracked.sum() >= 3 and (nxt[0, :n[0]][tracked] != np.rint(nxt[0, :n[0]][tracked])).any()


def test_track_with_eps_zero_and_a_loose_eigenvalue_bound(ctx, scene):
    """eps = 0 stops on a zero step, the oscillation rule or the count alone; min_eig = 0 leaves the det == 0 test alone.  The
    counts 1, 2 and 30 hold the kernel's shortcut to the rule: once a guess rounds to the position its step was taken from, the
    kernel does not run the iterations that would repeat that step (the reference does)."""
    s = scene
    for half, levels, eps, min_eig, max_iter in ((4, 3, 0.0, 1e-4, 6), (3, 2, 0.0, 0.0, 4), (5, 1, 0.03, 1e-2, MAX_ITER),
                                                 (4, 2, 0.0, 1e-4, 30), (2, 3, 0.01, 1e-4, 30), (4, 1, 0.0, 1e-4, 1), (4, 1, 0.0, 1e-4, 2)):
        got = _device_track(ctx, s["gray"], levels, s["pts"], s["n"], half, max_iter=max_iter, eps=eps, min_eig=min_eig)
        _assert_equal(got, _reference(s, levels, s["n"], half, max_iter=max_iter, eps=eps, min_eig=min_eig), s["n"], (half, levels))


def test_track_with_the_initial_flow_flag(ctx, scene):
    s = scene
    rng = np.random.default_rng(5)
    guess = (s["pts"] + np.float32(1.0) + rng.uniform(-1, 1, s["pts"].shape)).astype(np.float32)
    guess[2, 7] = np.nan, 3.0                                     # a non-finite guess: status 0, next = prev
    guess[:, CAP - 3:] = SENTINEL
    for half, levels in ((4, 3), (2, 1)):
        got = _device_track(ctx, s["gray"], levels, s["pts"], s["n"], half, guess=guess)
        _assert_equal(got, _reference(s, levels, s["n"], half, guess=guess, max_iter=MAX_ITER), s["n"], (half, levels))
        assert got[1][2, 7] == 0 and np.array_equal(_u32(got[0][2, 7]), _u32(s["pts"][2, 7]))
    plain = _device_track(ctx, s["gray"], 1, s["pts"], s["n"], 2)
    assert not np.array_equal(_u32(plain[0]), _u32(got[0]))        # (the guesses did act)


def test_track_under_a_row_range_ignores_the_rows_outside(ctx, scene):
    s = scene
    outs = []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        gray = s["gray"].copy()
        for i in range(NIMG):
            r0, r1 = ROW_RANGE[i // 2]
            gray[i, :r0] = rng.integers(0, 256, (r0, COLS))
            gray[i, r1:] = rng.integers(0, 256, (ROWS - r1, COLS))
        outs.append(_device_track(ctx, gray, 3, s["pts"], s["n"], 4, row_range=ROW_RANGE))
    want = _reference(s, 3, s["n"], 4, row_range=ROW_RANGE, max_iter=MAX_ITER)
    _assert_equal(outs[0], want, s["n"], "noise 1")
    _assert_equal(outs[1], want, s["n"], "noise 2")
    plain = _device_track(ctx, s["gray"], 3, s["pts"], s["n"], 4)
    assert not np.array_equal(plain[1], outs[0][1])                # (the range did act: starts above row 21 are lost)
    # a range that is empty or lies off the image is cut to the image: no read leaves it
    for bad in (np.array([[0, 0], [0, 0]], np.int32), np.array([[100, 200], [-5, -1]], np.int32)):
        got = _device_track(ctx, s["gray"], 3, s["pts"], s["few"], 4, row_range=bad)
        _assert_equal(got, _reference(s, 3, s["few"], 4, row_range=bad, max_iter=MAX_ITER), s["few"], bad.tolist())


@pytest.mark.parametrize("half,levels", [(4, 3), (2, 1), (10, 2)])
def test_track_with_the_forward_backward_check(ctx, scene, half, levels):
    s = scene
    n = s["few"] if half == 10 else s["n"]
    got = _device_track(ctx, s["gray"], levels, s["pts"], n, half, fb_max=0.25)
    _assert_equal(got, _reference(s, levels, n, half, fb_max=0.25, max_iter=MAX_ITER), n, (half, levels))
    fwd = _device_track(ctx, s["gray"], levels, s["pts"], n, half)
    assert np.array_equal(_u32(fwd[0]), _u32(got[0])) and np.array_equal(_u32(fwd[2]), _u32(got[2]))
    assert ((got[1] == 0) | (fwd[1] == got[1])).all()              # the check only clears


def test_rows_at_and_beyond_the_count_are_untouched(ctx, scene):
    s = scene
    got = _device_track(ctx, s["gray"], 3, s["pts"], s["n"], 4, fb_max=0.25)
    for p, c in enumerate(COUNTS):
        assert (_u32(got[0][p, c:]) == _u32(SENTINEL)).all() and (got[1][p, c:] == 0xA5).all()
        assert (_u32(got[2][p, c:]) == _u32(SENTINEL)).all() and (_u32(got[3][p, c:]) == _u32(SENTINEL)).all()
        assert (got[1][p, :c] <= 1).all()


def test_problems_in_swapped_order_give_swapped_results(ctx, scene):
    """prev_img / next_img: the problems name their images; an index off the set leaves its problem untouched."""
    s = scene
    a = _device_track(ctx, s["gray"], 3, s["pts"], s["n"], 4)
    order = [2, 3, 0, 1]
    b = _device_track(ctx, s["gray"], 3, s["pts"][order], s["n"][order], 4, prev_img=[PREV_IMG[i] for i in order],
                      next_img=[NEXT_IMG[i] for i in order])
    for x, y in zip(a, b):
        assert np.array_equal(x[order].view(np.uint8), y.view(np.uint8))
    c = _device_track(ctx, s["gray"], 3, s["pts"], s["n"], 4, prev_img=(0, 2, NIMG, 2), next_img=(1, -1, 1, 3))
    for x, y in zip(a, c):
        assert np.array_equal(x[[0, 3]].view(np.uint8), y[[0, 3]].view(np.uint8))
    assert (c[1][1:3] == 0xA5).all() and (_u32(c[0][1:3]) == _u32(SENTINEL)).all()


@pytest.mark.parametrize("half,levels,shift,bound", [(4, 1, SMALL_SHIFT, RECOVERED_SMALL), (4, 3, LARGE_SHIFT, RECOVERED_LARGE)])
def test_planted_shifts_are_recovered_on_the_device(ctx, half, levels, shift, bound):
    """The scenes and bounds of tests/test_lk_reference.py (twice the reference's largest error there: 0.06100 / 0.06960 px)."""
    gray = np.stack([reflk.texture(11, ROWS, COLS), reflk.texture(11, ROWS, COLS, shift)])
    pts = reflk.grid_points(ROWS, COLS, 24, 8)
    n = len(pts)
    buf = np.zeros((1, CAP, 2), np.float32)
    buf[0, :n] = pts
    nxt, st, _ = _device_track(ctx, gray, levels, buf, np.array([n], np.int32), half, prev_img=[0], next_img=[1])
    err = np.abs(nxt[0, :n].astype(np.float64) - pts - np.array(shift)).max()
    print("shift %s, half %d, %d levels: largest error on the device %.5f px (bound %.5f)" % (shift, half, levels, err, bound))
    assert st[0, :n].all() and err <= bound


def test_the_stages_refuse_bad_arguments(ctx):
    lib = _lib.load()
    gray = torch.zeros((2, 16, 16), dtype=torch.uint8, device=ctx.device)
    upper = torch.zeros((_lib.gray_pyramid_bytes(2, 16, 16, 4),), dtype=torch.uint8, device=ctx.device)
    pts = torch.zeros((1, 4, 2), dtype=torch.float32, device=ctx.device)
    st = torch.zeros((1, 4), dtype=torch.uint8, device=ctx.device)
    err = torch.zeros((1, 4), dtype=torch.float32, device=ctx.device)
    i32 = torch.zeros((1,), dtype=torch.int32, device=ctx.device)
    rr = torch.zeros((2, 2), dtype=torch.int32, device=ctx.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def pyramid(nimg=2, rows=16, cols=16, levels=3, row_range=None, out=upper):
        return lib.sosvo_gray_pyramid(ctx._h, p(gray), nimg, rows, cols, levels, row_range, None if out is None else p(out))

    def track(nimg=2, levels=3, cap=4, half=4, max_iter=10, eps=0.01, min_eig=1e-4, flags=0, back=None, fb_max=0.0, pyr=upper,
              row_range=None, nprob=1):
        return lib.sosvo_track_lk(ctx._h, p(gray), None if pyr is None else p(pyr), nimg, 16, 16, levels, row_range, p(i32), p(i32),
                                  nprob, cap, p(pts), p(i32), half, max_iter, eps, min_eig, flags, p(pts), p(st), p(err), back, fb_max)
    assert pyramid() == 0 and track() == 0 and pyramid(levels=1, out=None) == 0 and track(levels=1, pyr=None) == 0
    for bad in (dict(levels=0), dict(levels=5), dict(rows=0), dict(cols=16385), dict(out=None), dict(nimg=-1),
                dict(nimg=1, row_range=p(rr))):
        assert pyramid(**bad) == -1, bad
        assert "sosvo_gray_pyramid" in lib.sosvo_last_error(ctx._h).decode()
    for bad in (dict(half=1), dict(half=11), dict(max_iter=0), dict(max_iter=31), dict(eps=-0.1), dict(eps=float("nan")),
                dict(min_eig=-1.0), dict(cap=0), dict(cap=4097), dict(levels=0), dict(levels=5), dict(flags=2), dict(pyr=None),
                dict(back=p(pts), fb_max=0.0), dict(back=p(pts), fb_max=float("nan")), dict(nimg=1, row_range=p(rr)),
                dict(nprob=-1)):
        assert track(**bad) == -1, bad
        assert "sosvo_track_lk" in lib.sosvo_last_error(ctx._h).decode()
    out = ctypes.c_int64(-1)
    assert lib.sosvo_gray_pyramid_bytes(None, 2, 16, 16, 5, ctypes.byref(out)) == -1 and out.value == -1
    with pytest.raises(_lib.SosvoError):
        ctx.gray_pyramid(gray, 5)
    with pytest.raises(_lib.SosvoError):
        ctx.track_lk(None, i32, i32, pts, i32)
    ctx.synchronize()


# ---- the tracked assemble ----------------------------------------------------------------------------------------------------
def test_tracked_assemble_equals_a_numpy_restatement(ctx):
    """3 pairs over 3 frames, frame_cap 8, corr_cap 9: pair 0 has a lost point and a gated one per view, pair 1 names a frame
    with zero points, pair 2 has more survivors than corr_cap.  f is checked against Context.pano_to_bearing, the same device
    code behind its own entry point."""
    rng = np.random.default_rng(41)
    _, rig_kw = scenes.rig()
    F, Fc, Cc, NP = 3, 8, 9, 3
    cols, rows = rig_kw["pano_top"][0], rig_kw["pano_top"][1]
    m = [np.stack([rng.uniform(40, cols - 40, (F, Fc)), rng.uniform(8, rows - 8, (F, Fc))], -1).astype(np.float32) for _ in range(2)]
    X = rng.uniform(-3000, 3000, (F, Fc, 3))
    M = np.array([6, 0, 8], np.int32)
    ref = np.array([0, 1, 2], np.int32)
    trk = [(m[v][ref] + rng.uniform(-6, 6, (NP, Fc, 2))).astype(np.float32) for v in range(2)]
    st = [np.ones((NP, Fc), np.uint8) for _ in range(2)]
    st[0][0, 1], st[1][0, 4] = 0, 0                              # lost
    trk[0][0, 3, 0] = m[0][0, 3, 0] + 31.0                       # gated: |du| > 30
    trk[1][0, 0, 0] = m[1][0, 0, 0] - 30.5
    st[0][0, 7] = 1                                              # beyond M[0] = 6: never read
    frames = dict(m_top=_dev(ctx, m[0]), m_bot=_dev(ctx, m[1]), X=_dev(ctx, X), M=_dev(ctx, M))
    for hdiff in (30.0, -1.0):
        rig = make_rig(**dict(rig_kw, f2f_max_hdiff=hdiff))
        out = ctx.f2f_assemble_tracked(rig, frames, _dev(ctx, ref), _dev(ctx, trk[0]), _dev(ctx, trk[1]), _dev(ctx, st[0]),
                                       _dev(ctx, st[1]), Cc)
        ctx.synchronize()
        got = {k: v.cpu().numpy() for k, v in out.items()}
        for pr in range(NP):
            rows_, nt = [], min(int(M[ref[pr]]), Fc)
            for v in range(2):
                for k in range(nt):
                    du = abs(float(m[v][ref[pr], k, 0]) - float(trk[v][pr, k, 0]))
                    if st[v][pr, k] and (hdiff < 0 or du <= hdiff):
                        rows_.append((v, k))
                if v == 0:
                    n_top = min(len(rows_), Cc)
            rows_ = rows_[:Cc]
            assert got["n"][pr] == len(rows_) and got["n_top"][pr] == n_top, (pr, hdiff)
            assert [(int(c), int(t)) for c, t in zip(got["cam"][pr, :len(rows_)], got["t"][pr, :len(rows_)])] == rows_
            assert (got["q"][pr, :len(rows_)] == -1).all()
            for i, (v, k) in enumerate(rows_):
                assert np.array_equal(got["p"][pr, i], X[ref[pr], k])
                pano = rig_kw["pano_top" if v == 0 else "pano_bot"]
                b = ctx.pano_to_bearing(_dev(ctx, trk[v][pr, k].astype(np.float64).reshape(1, 2)), *pano)[2]
                assert np.array_equal(got["f"][pr, i], b.cpu().numpy()[0])
        assert got["n"][1] == 0 and got["n"][2] == Cc
    assert got["n"][0] == Cc and got["n_top"][0] == 5               # gate off: only the lost points are missing (5 + 5, cut to 9)


# ---- the pair pipeline ---------------------------------------------------------------------------------------------------------
def test_pair_pipeline_tracks_with_lk(ctx):
    """Pairs 0 and 1 of the rendered scene tests/test_gpu_cross_check.py uses (seed 99, GFT 330 features), one-mirror P3P with 500
    fixed iterations.  The tracker runs, RANSAC finds a model, and the figures are printed beside the matcher's.  The one
    condition on accuracy: the rotation error stays below the reference's own 5-degree inlier threshold."""
    B = 2
    gs, rig_kw = scenes.rig()
    omni, poses = synthetic.make_frame_pairs(gs, B, seed=99)
    model = DeviceImageModel(ctx, gs, (480, 640))
    fe = ImageFrontEnd(ctx, model, 2 * B, detection_method="GFT", num_of_features=330, keep_panoramas=False)
    fe.load_frames(omni)
    fe.run()
    for name, kw in (("match", {}), ("lk half 4", dict(f2f_tracker="lk", lk=dict(half=4, max_iter=10))),
                     ("lk half 10 + fb", dict(f2f_tracker="lk", lk=dict(half=10, max_iter=10, fb_max=0.5)))):
        pipe = FramePairPipeline(ctx, RigConfig(**rig_kw), B, frame_cap=2048, max_iter=500, seed=5, front_end=fe, **kw)
        pipe.stereo()
        pipe.track()
        rec = pipe.results().cpu().numpy()
        rot = [np.degrees(synth.pose_error(rec[i, :12].reshape(3, 4), R, t)[0]) for i, (R, t) in enumerate(poses)]
        trans = [np.linalg.norm(rec[i, 3:12:4] - t) for i, (R, t) in enumerate(poses)]
        print("%-16s inliers / correspondences %d / %d = %.3f, rotation error %s deg, translation error %s mm" % (
            name, rec[:, 12].sum(), rec[:, 13].sum(), rec[:, 12].sum() / max(rec[:, 13].sum(), 1),
            ["%.3f" % r for r in rot], ["%.1f" % t for t in trans]))
        assert (rec[:, 14] == 0).all(), name
        assert max(rot) < 5.0, name
        if kw:
            co = {k: v.cpu().numpy() for k, v in pipe.corr.items()}
            assert (co["n"] > 0).all() and (co["q"][0, :co["n"][0]] == -1).all()
            assert (np.diff(co["t"][0, :co["n_top"][0]]) > 0).all()          # point order within a view


# ---- the host mirror -----------------------------------------------------------------------------------------------------------
def test_host_mirror_returns_what_the_context_returns(ctx, scene):
    s = scene
    pts = s["pts"][0, :COUNTS[0]]
    nxt, st, err = common_cv.calc_optical_flow_pyr_lk(s["gray"][0], s["gray"][1], pts.reshape(-1, 1, 2), win_half=4, max_level=2,
                                                      max_iter=MAX_ITER, ctx=ctx)
    assert nxt.shape == (80, 1, 2) and st.shape == (80, 1) and err.shape == (80, 1)
    assert nxt.dtype == np.float32 and st.dtype == np.uint8 and err.dtype == np.float32
    want = _device_track(ctx, s["gray"][:2], 3, s["pts"][:1], s["n"][:1], 4, prev_img=[0], next_img=[1])
    assert np.array_equal(_u32(nxt[:, 0]), _u32(want[0][0, :80])) and np.array_equal(st[:, 0], want[1][0, :80])
    assert np.array_equal(_u32(err[:, 0]), _u32(want[2][0, :80]))
    guess = nxt + np.float32(0.25)
    again = common_cv.calc_optical_flow_pyr_lk(s["gray"][0], s["gray"][1], pts, next_pts=guess, win_half=4, max_level=0, ctx=ctx)
    assert again[0].shape == (80, 1, 2) and again[1].sum() > 40
    with pytest.raises(ValueError):
        common_cv.calc_optical_flow_pyr_lk(s["gray"][0], s["gray"][1], pts, win_half=11, ctx=ctx)
    empty = common_cv.calc_optical_flow_pyr_lk(s["gray"][0], s["gray"][1], np.zeros((0, 1, 2), np.float32), ctx=ctx)
    assert empty[0].shape == (0, 1, 2)
