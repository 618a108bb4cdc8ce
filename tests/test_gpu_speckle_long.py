"""GPU: the speckle filter at the extents its small tests do not reach: four and 64 rounds of the row
kernel (a buffer of last breaks reused, a break carried over many rounds), the row and column limits, the working size (822
workgroups per frame, a component above 65535 pixels) and one call of 201 frames.  The device reproduces tests/refspeckle.py --
labels and map -- bit for bit on the maps of tests/speckle_long_cases.py, n = 3 frames of different content per call.
array_equal throughout."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refspeckle  # noqa: E402
import speckle_long_cases as cases  # noqa: E402
from test_gpu_speckle import _dev, _ref_map, _run  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_DIFFS = (0, 16, 32767)
N_BATCHES = 5
_LABELS = {}


def _ref_labels(key, d, max_diff, cyclic):
    """refspeckle's labels of the frames d, computed once per (batch, max_diff, cyclic)."""
    key = key + (max_diff, cyclic)
    if key not in _LABELS:
        _LABELS[key] = np.stack([refspeckle.labels_of(f, max_diff, cyclic) for f in d])
    return _LABELS[key]


def _compare(ctx, key, names, d, want_exact_above=0):
    rows, cols = d.shape[1:]
    t = _dev(ctx, d)
    for cyclic in (False, True):
        for max_diff in MAX_DIFFS:
            want_lab = _ref_labels(key, d, max_diff, cyclic)
            # a component's exact size (dropped) and one less (kept): the largest component of the batch's first frame
            counts = np.unique(want_lab[0][want_lab[0] != refspeckle.NONE], return_counts=True)[1]
            exact = int(counts.max()) if len(counts) else 2
            assert exact > want_exact_above, (names, exact)
            for max_size in (0, 1, exact, exact - 1, rows * cols):
                got, lab = _run(ctx, t, max_size, max_diff, cyclic, want_labels=True)
                where = (names[:3], cyclic, max_diff, max_size)
                assert np.array_equal(lab, want_lab), ("labels",) + where + (np.argwhere(lab != want_lab)[:5].tolist(),)
                want = _ref_map(d, want_lab, max_size)
                assert np.array_equal(got, want), ("map",) + where + (np.argwhere(got != want)[:5].tolist(),)
                if max_size == 0:
                    assert np.array_equal(got, d)
                if max_size == rows * cols:
                    assert (got < 0).all() and np.array_equal(got[d < 0], d[d < 0])
                if max_size in (exact, exact - 1) and len(counts):
                    big = want_lab[0] == np.unique(want_lab[0][want_lab[0] != refspeckle.NONE])[counts.argmax()]
                    assert (got[0][big] == -1).all() if max_size == exact else np.array_equal(got[0][big], d[0][big])
    del t


@pytest.mark.parametrize("batch", range(N_BATCHES))
@pytest.mark.parametrize("shape", cases.SHAPES, ids=lambda s: "%dx%d" % s)
def test_map_and_labels_equal_the_numpy_statement(ctx, shape, batch):
    batches = cases.batches(*shape)
    assert len(batches) == N_BATCHES
    names, d = batches[batch]
    # at the working size the batch that begins with `constant` holds one component of the whole frame: more than a u16 counts
    above = 65535 if shape == (146, 1440) and batch == 3 else 0
    assert (names[0] == "constant") == (batch == 3)
    _compare(ctx, (shape, batch), names, d, above)


def test_one_call_of_201_frames(ctx):
    names, d = cases.many()
    assert d.shape == (201, 3, 5)
    _compare(ctx, ("many",), names, d)


@pytest.mark.parametrize("shape", cases.SHAPES + [cases.MANY], ids=lambda s: "x".join("%d" % v for v in s))
def test_in_place_equals_out_of_place(ctx, shape):
    names, d = cases.many() if len(shape) == 3 else cases.batches(*shape)[N_BATCHES - 1]
    for cyclic in (False, True):
        want, want_lab = refspeckle.speckle(d, 6, 16, cyclic, want_labels=True)
        t = _dev(ctx, d)
        plain = _run(ctx, t, 6, 16, cyclic)                              # out of place, labels_out NULL
        assert np.array_equal(t.cpu().numpy(), d), "the input was written"
        t2 = _dev(ctx, d)
        same = ctx.dense_speckle(t2, options=dict(max_size=6, max_diff=16, cyclic=cyclic), out=t2)     # in place
        ctx.synchronize()
        assert same is t2
        t3 = _dev(ctx, d)
        in_place_lab = _run(ctx, t3, 6, 16, cyclic, want_labels=True, out=t3)[1]
        for got in (plain, t2.cpu().numpy(), t3.cpu().numpy()):
            assert np.array_equal(got, want), (names[:3], cyclic, np.argwhere(got != want)[:5].tolist())
        assert np.array_equal(in_place_lab, want_lab)
