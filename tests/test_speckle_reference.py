"""CPU: tests/refspeckle.py -- the numpy statement of the speckle filter -- pinned against things it was
not written from: scipy.ndimage.label, a flood fill with an explicit stack (the manner of cv2.filterSpeckles), ray-cast truth
of synthetic.Room; and SpeckleOptions, which needs no GPU.  The thresholds are conditions on the reference alone; the measured
values stand beside them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refspeckle  # noqa: E402
import speckle_cases  # noqa: E402

IDS = ["%dx%d" % s for s in speckle_cases.SHAPES]


def _flood_fill(d16, max_size, max_diff, cyclic):
    """One frame -> (map, labels relabelled to the smallest index of the component): pixels in row-major order, each
    unlabelled valid pixel the seed of a fill over an explicit stack."""
    rows, cols = d16.shape
    d = d16.astype(np.int64).tolist()
    label = [[-1] * cols for _ in range(rows)]
    out = d16.copy()
    for r0 in range(rows):
        for c0 in range(cols):
            if d[r0][c0] < 0 or label[r0][c0] >= 0:
                continue
            seed = r0 * cols + c0          # (row-major order: the seed is the component's smallest index)
            label[r0][c0] = seed
            stack, members = [(r0, c0)], []
            while stack:
                r, c = stack.pop()
                members.append((r, c))
                around = [(r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1)]
                if cyclic and cols > 1:
                    around = [(rr, cc % cols) for rr, cc in around]
                for rr, cc in around:
                    if 0 <= rr < rows and 0 <= cc < cols and d[rr][cc] >= 0 and label[rr][cc] < 0 \
                            and abs(d[rr][cc] - d[r][c]) <= max_diff:
                        label[rr][cc] = seed
                        stack.append((rr, cc))
            if len(members) <= max_size:
                for r, c in members:
                    out[r, c] = -1
    lab = np.array(label, dtype=np.int64)
    return out, np.where(lab < 0, 0xFFFFFFFF, lab).astype(np.uint32)


@pytest.mark.parametrize("shape", speckle_cases.SHAPES, ids=IDS)
def test_sizes_equal_scipys_label_when_every_valid_pair_is_joined(shape):
    """max_diff 32767 joins every pair of valid neighbours: the components are those of scipy.ndimage.label (4-connected) on
    d16 >= 0; for the cyclic form after merging the labels that face each other across the seam."""
    from scipy import ndimage
    names, d = speckle_cases.frames(*shape)
    rows, cols = shape
    for name, f in zip(names, d):
        for cyclic in (False, True):
            _, lab = refspeckle.speckle(f, 0, 32767, cyclic, want_labels=True)
            theirs, count = ndimage.label(f >= 0, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
            if cyclic and cols > 1:
                alias = np.arange(count + 1)
                for r in range(rows):
                    a, b = theirs[r, 0], theirs[r, cols - 1]
                    if a and b:
                        lo, hi = sorted((alias[a], alias[b]))
                        alias[alias == hi] = lo
                theirs = alias[theirs]
            valid = f >= 0
            assert np.array_equal(lab != refspeckle.NONE, valid), name
            # the same partition: each of our labels meets exactly one of theirs and the other way round
            pairs = np.unique(np.stack([lab[valid].astype(np.int64), theirs[valid]]), axis=1)
            assert len(np.unique(pairs[0])) == pairs.shape[1] == len(np.unique(pairs[1])), (name, cyclic)
            ours = np.sort(np.unique(lab[valid], return_counts=True)[1])
            assert np.array_equal(ours, np.sort(np.unique(theirs[valid], return_counts=True)[1])), (name, cyclic)


@pytest.mark.parametrize("shape", speckle_cases.SHAPES, ids=IDS)
def test_map_and_labels_equal_a_flood_fill(shape):
    names, d = speckle_cases.frames(*shape)
    for max_size, max_diff, cyclic in ((100, 16, False), (100, 16, True), (3, 15, True), (1, 0, False), (40, 32767, True)):
        got, lab = refspeckle.speckle(d, max_size, max_diff, cyclic, want_labels=True)
        for k, name in enumerate(names):
            want, want_lab = _flood_fill(d[k], max_size, max_diff, cyclic)
            assert np.array_equal(lab[k], want_lab), (name, max_size, max_diff, cyclic)
            assert np.array_equal(got[k], want), (name, max_size, max_diff, cyclic)


def test_the_cases_are_what_their_names_say():
    """One component for the ramp, the serpentine and the comb; size 1 everywhere on the checkerboard; the seam cases change
    with `cyclic`; the non-transitive ramp of the header: 0, 16, 32, 48 is one component under max_diff 16, four under 15."""
    names, d = speckle_cases.frames(12, 9)
    f = dict(zip(names, d))

    def sizes(name, max_diff, cyclic=False):
        lab = refspeckle.labels_of(f[name], max_diff, cyclic)
        return sorted(np.unique(lab[lab != refspeckle.NONE], return_counts=True)[1].tolist())
    assert sizes("ramp", 16) == [108] and sizes("ramp", 15) == [1] * 108
    assert sizes("checkerboard", 16) == [1] * 108 and sizes("constant", 0) == [108]
    assert sizes("serpentine", 16) == [6 * 9 + 6] and sizes("comb", 16) == [11 * 5 + 9]
    assert len(sizes("seam_blobs", 16)) == 2 and len(sizes("seam_blobs", 16, True)) == 1
    assert sizes("ring", 16) == [4, 4, 9] and sizes("ring", 16, True) == [8, 9] and sizes("ring", 15, True) == [4, 4, 9]
    assert sizes("all_invalid", 32767, True) == []
    ramp = np.array([[0, 16, 32, 48]], np.int16)
    assert np.array_equal(refspeckle.speckle(ramp, 3, 16), ramp) and (refspeckle.speckle(ramp, 4, 16) == -1).all()
    assert (refspeckle.speckle(ramp, 1, 15) == -1).all() and np.array_equal(refspeckle.speckle(ramp, 0, 15), ramp)
    keep = np.array([[-2, 5, -32768, 7, 7]], np.int16)          # invalid values pass through, whatever they are
    assert np.array_equal(refspeckle.speckle(keep, 1, 0), [[-2, -1, -32768, 7, 7]])
    assert np.array_equal(refspeckle.speckle(keep, 1, 0, cyclic=True), [[-2, -1, -32768, 7, 7]])


def test_ray_cast_truth_of_the_near_room():
    """The near room of tests/test_dense_reference.py (width 640, 65 rows, ksize 11), max_size 100, max_diff 16, cyclic.
    Required: at least 0.80 of the removed comparable pixels were wrong by more than one row, the within-one-row share rises by
    at least 0.008, the valid share falls by at most 0.025.
    Measured: 516 comparable pixels removed, 0.897 of them wrong; within 1 row 0.9056 -> 0.9195 (+0.0139); valid 0.9024 ->
    0.8869 (-0.0155); median 0.3000 -> 0.2944."""
    import refdense
    import test_dense_reference as tdr
    from vo_single_camera_sos_amd import synthetic
    d16, true, valid = tdr._ray_cast_case(640, synthetic.Room(seed=3, half_x=(500.0, 1500.0), half_y=(400.0, 2500.0)), 11)
    out = refspeckle.speckle(d16, 100, 16, cyclic=True)
    comparable, share0, within0, med0 = refdense.accuracy(d16, true, valid[0], valid[1])
    _, share1, within1, med1 = refdense.accuracy(out, true, valid[0], valid[1])
    rows, cols = true.shape
    rr, cc = np.mgrid[0:rows, 0:cols]
    rb = np.clip(np.rint(rr - true).astype(np.int64), 0, rows - 1)          # (refdense.accuracy's comparable pixels)
    comp = (valid[0] != 0) & (valid[1][rb, cc] != 0) & (rr - true >= 0) & (true < 63)
    assert int(comp.sum()) == comparable
    removed = comp & (d16 >= 0) & (out < 0)
    wrong = float((np.abs(d16[removed] / 16.0 - true[removed]) > 1.0).mean())
    print("near room: %d comparable pixels removed, %.4f of them wrong; within 1 row %.4f -> %.4f (%+.4f); valid %.4f -> %.4f (%+.4f); "
          "median %.4f -> %.4f" % (removed.sum(), wrong, within0, within1, within1 - within0, share0, share1, share1 - share0, med0, med1))
    assert np.array_equal(out[out >= 0], d16[out >= 0]) and (d16[out < 0] >= -1).all()
    assert wrong >= 0.80 and within1 - within0 >= 0.008 and share0 - share1 <= 0.025


def test_speckle_options_refuse_every_bad_value():
    from vo_single_camera_sos_amd._lib import DenseOptions, SpeckleOptions, StepOptions
    o = SpeckleOptions()
    assert tuple(o) == (100, 16, False) and o.flags == 0 and SpeckleOptions(cyclic=True).flags == 1
    assert SpeckleOptions(0, 0) == (0, 0, False) and SpeckleOptions((1 << 31) - 1, 32767, True) == ((1 << 31) - 1, 32767, True)
    assert SpeckleOptions(max_size=5.0).max_size == 5 and isinstance(SpeckleOptions(max_size=5.0).max_size, int)
    assert SpeckleOptions.of(None) is None and SpeckleOptions.of(o) is o
    assert SpeckleOptions.of(dict(max_size=7, cyclic=True)) == (7, 16, True)
    assert hash(o) == hash(SpeckleOptions()) and {o: 1}[SpeckleOptions(100, 16)] == 1 and o != SpeckleOptions(cyclic=True)
    assert SpeckleOptions.from_tuner(0, 3) is None and SpeckleOptions.from_tuner(0, 0, cyclic=True) is None
    assert SpeckleOptions.from_tuner(100, 1) == (100, 16, False) and SpeckleOptions.from_tuner(50, 2, cyclic=True) == (50, 32, True)
    bad = [dict(max_size=True), dict(max_diff=False), dict(max_size=1.5), dict(max_diff=0.5), dict(max_size=float("nan")),
           dict(max_diff=float("nan")), dict(max_size=-1), dict(max_diff=-1), dict(max_diff=32768), dict(max_size=1 << 31),
           dict(max_size=None), dict(max_diff="16"), dict(cyclic=2), dict(cyclic="yes")]
    for kw in bad:
        with pytest.raises(ValueError):
            SpeckleOptions(**kw)
    for value in (dict(size=3), dict(max_size=3, window=1), 7, (100, 16, False), "on"):
        with pytest.raises(ValueError):
            SpeckleOptions.of(value)
    for args in ((-1, 1), (1.5, 1), (True, 1), (100, 2048), (100, -1), (100, 0.5), (100, True), (100, float("nan"))):
        with pytest.raises(ValueError):
            SpeckleOptions.from_tuner(*args)
    assert len(tuple(DenseOptions())) == 6 and tuple(DenseOptions()) == (1, 8, 48, 15, 1, False)
    assert "speckle" not in StepOptions._fields and "speckle" not in DenseOptions._fields
