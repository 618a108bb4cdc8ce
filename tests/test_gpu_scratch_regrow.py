"""GPU: a stage's pointers into the context's scratch come from the scratch as it is AFTER the stage reserved its size.
ONE context runs eight stage entry points in an order in which every call needs more scratch than the one before, so every
call frees the allocation and makes a new one (sosvo_ws_reserve); a layout placed over the base from before the reserve would
write through a freed pointer.  Scratch totals of the calls below (bytes, from each stage's layout; csrc/scratch_carver.h):

    1. sosvo_dense_speckle        9 x 16, n = 1                               1 536
    2. sosvo_ransac_rel_pose      1 problem, stride 32, 16 iterations         1 792
    3. sosvo_refine_stereo_lk     two 24 x 32 images, 1 mask, cap 16          2 048
    4. sosvo_detect_fast          40 x 64                                     3 072
    5. sosvo_ransac_abs_pose      2 problems, stride 64, 256 iterations      73 472
    6. sosvo_detect_describe_orb  96 x 128, 2 masks                         137 472
    7. sosvo_detect_gft           40 x 64, 2 images, 2 masks                146 176
    8. sosvo_dense_stereo         32 x 64, n = 2                            872 448

(the corner detector's candidate records have room for every pixel of every strip, so at these sizes it comes after the two
that a first guess would put behind it).  The scratch is filled with 0xFF between the calls, every output must equal, bit for bit, that of the same call on a fresh
context, and then the same calls run in reverse order on the grown context (no call reallocates) for the same equality."""
import numpy as np
import pytest
import torch

import reflk
from vo_single_camera_sos_amd import _lib, orb_pattern
from vo_single_camera_sos_amd.device import Context

pytestmark = pytest.mark.gpu


def _bits(sets, rows, cols, nmask):
    """mask_bits [sets, rows, cols] u32: mask m of set s is a band of columns, the bands overlap by a few columns."""
    x = np.arange(cols)
    bits = np.zeros((sets, rows, cols), np.uint32)
    for s in range(sets):
        for m in range(nmask):
            lo, hi = m * cols // nmask - 3 - s, (m + 1) * cols // nmask + 3
            bits[s, :, (x >= lo) & (x < hi)] |= np.uint32(1 << m)
    return bits


def _bearings(rng, shape):
    v = rng.normal(size=shape + (3,)) + (0.0, 0.0, 4.0)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _stages(dev):
    """-> [(name, call)]: call(ctx) runs the stage on inputs made here once (never written) and returns its outputs."""
    rng = np.random.default_rng(2024)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    R = np.array([[np.cos(0.1), 0.0, np.sin(0.1)], [0.0, 1.0, 0.0], [-np.sin(0.1), 0.0, np.cos(0.1)]])
    tr = np.array([0.3, -0.1, 0.2])

    d16 = t(rng.choice(np.array([-1, 40, 44, 200], np.int16), size=(1, 9, 16), p=(0.2, 0.4, 0.3, 0.1)))
    speckle = lambda ctx: ctx.dense_speckle(d16, options=_lib.SpeckleOptions(max_size=3, max_diff=8, cyclic=False), want_labels=True)  # noqa: E731

    X = rng.uniform(-2.0, 2.0, (1, 32, 3)) + (0.0, 0.0, 6.0)
    f1 = t(X / np.linalg.norm(X, axis=-1, keepdims=True))
    X2 = (X - tr) @ R          # the points in frame 2 (x2 = R^T (x - t))
    f2, n_rel = t(X2 / np.linalg.norm(X2, axis=-1, keepdims=True)), t(np.array([30], np.int32))
    rel = lambda ctx: tuple(ctx.ransac_rel_pose(f1, f2, n_rel, 1e-6, 16, seed=5, want_counts=True).values())  # noqa: E731

    shift = (0.4, 2.3)
    gray_lk = t(np.stack([reflk.texture(3, 24, 32, waves=20, hi=16.0), reflk.texture(3, 24, 32, shift, waves=20, hi=16.0)]))
    kp_top = np.zeros((1, 16, 2), np.float32)
    kp_top[0, :6] = [(10, 9), (14.5, 10.25), (18, 12), (21, 13.5), (12, 14), (16, 11)]
    kp_bot = np.zeros((1, 16, 2), np.float32)
    kp_bot[0, :5] = np.rint(kp_top[0, [2, 0, 5, 1, 3]].astype(np.float64) + shift)
    keys = np.full((1, 16), 0xFFFFFFFF, np.uint32)
    keys[0, :5] = [2 | (7 << 20), 0 | (9 << 20), 5 | (1 << 20), 1 | (30 << 20), 3 | (2 << 20)]
    kp_top, keys, n_top, n_bot, kp_bot = t(kp_top), t(keys), t(np.array([6], np.int32)), t(np.array([5], np.int32)), t(kp_bot)
    slk = lambda ctx: ctx.refine_stereo_lk(gray_lk, kp_top, n_top, kp_bot.clone(), n_bot, keys, 1, stereo_lk=dict(half=3))  # noqa: E731

    noise = t(rng.integers(0, 256, (2, 40, 64), dtype=np.uint8))
    bits1, bits2 = t(_bits(1, 40, 64, 1)), t(_bits(2, 40, 64, 2))
    fast = lambda ctx: ctx.detect_fast(noise[:1], bits1, 1, 1, 64, threshold=10)  # noqa: E731
    gft = lambda ctx: ctx.detect_gft(noise, bits2, 1, 2, 32, quality=0.01, min_distance=3.0, max_corners=24)  # noqa: E731

    T = np.concatenate([R, tr[:, None]], 1)
    f_abs, p_abs = np.zeros((2, 64, 3)), np.zeros((2, 64, 3))
    for b in range(2):
        P3 = rng.uniform(-2.0, 2.0, (64, 3)) + (0.0, 0.0, 6.0)
        Xc = (P3 - T[:, 3]) @ T[:, :3]
        f_abs[b], p_abs[b] = Xc / np.linalg.norm(Xc, axis=-1, keepdims=True), P3
    f_abs[:, 50:] = _bearings(rng, (2, 14))          # outliers
    f_abs, p_abs, n_abs = t(f_abs), t(p_abs), t(np.array([64, 57], np.int32))
    ransac = lambda ctx: tuple(ctx.ransac_abs_pose(f_abs, p_abs, n_abs, 1e-5, 256, seed=9, want_counts=True).values())  # noqa: E731

    img = t(np.stack([reflk.texture(11, 96, 128, waves=60, lo=2.5, hi=12.0)]))
    bits_orb, pattern = t(_bits(1, 96, 128, 2)), t(orb_pattern.orb_pattern())
    mask_pyr = Context(dev.index).orb_mask_pyramid(bits_orb, 2)          # (no scratch: made once, outside the sequence)

    def orb(ctx):
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        return ctx.detect_describe_orb(img, mask_pyr, 1, 2, 40, pattern, z((2, 32, 4), torch.float32), z((2, 32), torch.float32),
                                       z((2,), torch.int32), z((2, 32, 32), torch.uint8), kp_xy=z((2, 32, 2), torch.float32))

    top = t(np.stack([reflk.texture(21 + k, 32, 64, waves=30, hi=20.0) for k in range(2)]))
    bot = t(np.stack([reflk.texture(21 + k, 32, 64, (0.0, -3.0 - k), waves=30, hi=20.0) for k in range(2)]))
    dense = lambda ctx: ctx.dense_stereo(top, bot, options=_lib.DenseOptions(0, 8, 32, 10, 1, False))  # noqa: E731
    return [("dense_speckle", speckle), ("ransac_rel_pose", rel), ("refine_stereo_lk", slk), ("detect_fast", fast),
            ("ransac_abs_pose", ransac), ("detect_describe_orb", orb), ("detect_gft", gft), ("dense_stereo", dense)]


def _host(ctx, out):
    ctx.synchronize()
    return [o.cpu().numpy().copy() for o in (out if isinstance(out, (tuple, list)) else (out,)) if o is not None]


def test_every_stage_places_its_buffers_in_the_scratch_it_has_just_grown():
    dev = torch.device("cuda", 0)
    stages = _stages(dev)
    want = {}
    for name, call in stages:          # each call on a context of its own
        fresh = Context(0)
        want[name] = _host(fresh, call(fresh))
        assert any(a.any() for a in want[name]), name          # (a result worth comparing)
    one = Context(0)
    for order in (stages, stages[::-1]):          # growing: every call reallocates; then shrinking, on the grown scratch
        for name, call in order:
            one.debug_fill_scratch(0xFF)
            got = _host(one, call(one))
            assert len(got) == len(want[name])
            for k, (g, w) in enumerate(zip(got, want[name])):
                assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (name, k, order is stages)
