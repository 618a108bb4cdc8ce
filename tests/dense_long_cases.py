"""The inputs on which dense omnistereo is tested at long axes, wide rows, large offsets and large
batches, for tests/test_dense_long_reference.py (conditions on the numpy statement alone) and tests/test_gpu_dense_long.py (the
device against the numpy statement), with the references computed once per session.  Textures as in tests/test_gpu_dense.py: a
smoothed random texture, the bottom view the top shifted by a planted number of rows (plus noise in +-3), seeded from the shape.
No GPU here."""
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refdense  # noqa: E402
from test_gpu_dense import OPTION_SETS, _mask, _texture  # noqa: E402

# one run of a case: opts = (P1, P2, uniqueness, lr_max, d0) as in test_gpu_dense.OPTION_SETS
Run = namedtuple("Run", "opts cyclic masked")
# frames: (planted shift in rows, noisy) per frame, None = a constant frame; every frame has a texture of its own unless
# `shared` (then the frames are cut from one texture, as test_gpu_dense._frames does)
Case = namedtuple("Case", "name rows cols frames shared runs")

DEFAULT = (8, 48, 15, 1, 0)


def _runs(option_sets, cyclics=(False, True), masks=(False,)):
    return [Run(o, c, m) for o in option_sets for c in cyclics for m in masks]


CASES = [
    # rows above 255: bits 8..13 of the row field of the left-right key; (8191, 8191, ..) makes mS and r large together
    Case("tall300", 300, 3, [(5, True), None, (63, False)], True, _runs(OPTION_SETS, masks=(False, True))),
    # the row limit
    Case("tall16384", 16384, 2, [(5, True), (63, False)], True,
         [Run((8, 48, 15, 1, 1), False, False), Run((50, 1000, 15, 0, 7), True, False)]),
    # min_disparity at its limit and near it: frame 0 answers d0 = 1024, frame 1 answers d0 = 1000
    Case("offset1024", 1300, 3, [(1064, True), (1010, True)], False, _runs([(8, 48, 15, 1, 1024), (8, 48, 15, 1, 1000)])),
    # min_disparity beyond the frame: every cost is 64, every pixel -1
    Case("offset_beyond", 40, 9, [(5, True), (7, True)], False, _runs([(8, 48, 15, 1, 1024)], masks=(False, True))),
    # three census column blocks, row paths of 700 steps
    Case("wide700", 12, 700, [(3, True), (3, True)], False, _runs([(8, 48, 15, 1, 0), (0, 0, 0, -1, 1)])),
    # the column limit
    Case("wide16384", 3, 16384, [(1, True), (1, True)], False, _runs([DEFAULT])),
    # blockIdx.y up to 129, a select wave of 64 pixels over more than four frames
    Case("many_small", 5, 3, [(1, True)] * 130, False, _runs([DEFAULT], masks=(False, True))),
    Case("many_single", 1, 1, [(0, False)] * 300, False, _runs([DEFAULT])),
    # the shipped shape; DenseOptions() with cyclic=True
    Case("working", 146, 1440, [(5, True), (20, False)], True, [Run((8, 48, 15, 1, 1), True, True), Run((8, 48, 15, 1, 1), True, False)]),
]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]

_FRAMES, _CENSUS, _S, _D16 = {}, {}, {}, {}


def frames(name):
    """-> top, bot [n, rows, cols] u8 (do not write to them)."""
    if name not in _FRAMES:
        case = BY_NAME[name]
        rows, cols = case.rows, case.cols
        rng = np.random.default_rng(rows * 1000 + cols)
        reach = max(f[0] for f in case.frames if f is not None)
        tall = _texture(rng, rows + reach, cols) if case.shared else None
        top, bot = [], []
        for f in case.frames:
            if f is None:
                top.append(np.full((rows, cols), 77, np.uint8))
                bot.append(np.full((rows, cols), 77, np.uint8))
                continue
            shift, noisy = f
            t = tall if case.shared else _texture(rng, rows + shift, cols)
            b = t[shift:shift + rows]
            if noisy:
                b = np.clip(b.astype(np.int32) + rng.integers(-3, 4, (rows, cols)), 0, 255).astype(np.uint8)
            top.append(t[:rows])
            bot.append(b)
        _FRAMES[name] = (np.ascontiguousarray(np.stack(top)), np.ascontiguousarray(np.stack(bot)))
    return _FRAMES[name]


def mask(name):
    case = BY_NAME[name]
    return _mask(case.rows, case.cols)


def ref_census(name, cyclic):
    """refdense's census words of both views [2 n, rows, cols] u64, computed once per (case, cyclic)."""
    key = (name, cyclic)
    if key not in _CENSUS:
        _CENSUS[key] = refdense.census(np.concatenate(frames(name)), cyclic)
    return _CENSUS[key]


def ref_S(name, d0, P1, P2, cyclic):
    """refdense's S of every frame [n, rows, cols, 64] u16, computed once per (case, d0, P1, P2, cyclic)."""
    key = (name, d0, P1, P2, cyclic)
    if key not in _S:
        cen = ref_census(name, cyclic)
        n = len(cen) // 2
        _S[key] = np.stack([refdense.aggregate(refdense.cost_volume(cen[k], cen[n + k], d0), P1, P2) for k in range(n)])
    return _S[key]


def ref_d16(name, run):
    """refdense's d16 of every frame [n, rows, cols] i16, computed once per (case, run)."""
    key = (name, run)
    if key not in _D16:
        P1, P2, uniq, lr_max, d0 = run.opts
        m = mask(name) if run.masked else None
        _D16[key] = np.stack([refdense.select(s, d0, uniq, lr_max, m) for s in ref_S(name, d0, P1, P2, run.cyclic)])
    return _D16[key]


def forget(name):
    """Drop the cached references of one case (the large ones, once their test has run)."""
    for cache in (_FRAMES, _CENSUS, _S, _D16):
        for key in [k for k in cache if (k if isinstance(k, str) else k[0]) == name]:
            del cache[key]
