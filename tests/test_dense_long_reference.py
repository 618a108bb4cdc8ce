"""CPU: the inputs of tests/dense_long_cases.py and tests/speckle_long_cases.py can tell a right kernel from a wrong one.
Conditions on tests/refdense.py and tests/refspeckle.py alone (the device is compared with them in test_gpu_dense_long.py and
test_gpu_speckle_long.py); the measured values stand beside them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_long_cases as cases  # noqa: E402
import refdense  # noqa: E402
import refspeckle  # noqa: E402
import speckle_long_cases  # noqa: E402


def _left_right_by_key(S, d0, uniqueness, lr_max, mask, bits):
    """refdense.select with the left-right step restated the device's way: every survivor offers (mS << bits) | r to its
    target, the smallest key wins, the kept row is key & (2**bits - 1).  -> (d16, d16 before the step, r, c and target row
    of the survivors)."""
    before = refdense.select(S, d0, uniqueness, -1, mask)
    S = S.astype(np.int64)
    ks, mS = S.argmin(axis=-1), S.min(axis=-1)
    r, c = np.nonzero(before >= 0)
    rb = r - (d0 + ks[r, c])
    best = np.full(before.shape, 0xFFFFFFFF, np.int64)
    np.minimum.at(best, (rb, c), (mS[r, c] << bits) | r)
    kept_row = best[rb, c] & ((1 << bits) - 1)
    bad = np.abs(ks[kept_row, c] - ks[r, c]) > lr_max
    out = before.copy()
    out[r[bad], c[bad]] = -1
    return out, before, (r, c, rb)


@pytest.mark.parametrize("name", ["tall300", "tall16384"])
def test_the_tall_cases_need_every_bit_of_the_row_field(name):
    """The key with 14 row bits is refdense.select on every run; with 8 bits it is not (13 bits: not at 16384 rows).
    Measured, pixels of the three or two frames that differ with 8 bits: tall300 without a mask and not cyclic, (8, 48, 15, 1, 0)
    146, (50, 1000, 15, 0, 7) 205, (8191, 8191, 99, 63, 0) none (lr_max 63 drops nothing); tall16384 (8, 48, 15, 1, 1) 8505,
    with 13 bits 135; (50, 1000, 15, 0, 7) 20863, with 13 bits 6964.  tall16384, (50, 1000, 15, 0, 7), frame 0: 853 targets claimed by two or more survivors of rows >= 8192, and the
    check drops 922 pixels of those rows."""
    case = cases.BY_NAME[name]
    differ = {8: 0, 13: 0}
    for run in case.runs:
        P1, P2, uniq, lr_max, d0 = run.opts
        if lr_max < 0:
            continue
        want = cases.ref_d16(name, run)
        mask = cases.mask(name) if run.masked else None
        by_run = {8: 0, 13: 0}
        for k, S in enumerate(cases.ref_S(name, d0, P1, P2, run.cyclic)):
            assert np.array_equal(_left_right_by_key(S, d0, uniq, lr_max, mask, 14)[0], want[k]), (run, k)
            for bits in by_run:
                by_run[bits] += int((_left_right_by_key(S, d0, uniq, lr_max, mask, bits)[0] != want[k]).sum())
        print(name, run, "differ with 8 / 13 row bits:", by_run[8], by_run[13])
        if lr_max < 63:                 # (lr_max 63 keeps every pixel, whichever row the key names)
            assert by_run[8] >= 1, run
            if case.rows > 8192:
                assert by_run[13] >= 1, run
        for bits in differ:
            differ[bits] += by_run[bits]
    assert differ[8] >= 1 and (case.rows <= 8192 or differ[13] >= 1)
    if name == "tall16384":
        run = case.runs[1]
        P1, P2, uniq, lr_max, d0 = run.opts
        S = cases.ref_S(name, d0, P1, P2, run.cyclic)[0]
        out, before, (r, c, rb) = _left_right_by_key(S, d0, uniq, lr_max, None, 14)
        high = r >= 8192
        claims = np.unique(rb[high] * case.cols + c[high], return_counts=True)[1]
        dropped = int(((before >= 0) & (out < 0))[8192:].sum())
        print("targets claimed twice from rows >= 8192:", int((claims >= 2).sum()), "dropped there:", dropped)
        assert (claims >= 2).sum() >= 1 and dropped >= 1


def test_offset1024_finds_its_planted_shifts():
    """Frame 0 (shift 1064) under d0 = 1024 and frame 1 (shift 1010) under d0 = 1000: the share of valid pixels is within 0.02
    of (rows - shift) / rows, the largest d16 within 16 of 16 shift, every valid pixel has r >= d0.
    Measured: 0.1826 (0.1815) and 17031 (17024); 0.2238 (0.2231) and 16166 (16160)."""
    case = cases.BY_NAME["offset1024"]
    for frame, (shift, d0) in enumerate(((1064, 1024), (1010, 1000))):
        assert case.frames[frame][0] == shift
        for run in case.runs:
            if run.opts[4] != d0:
                continue
            d16 = cases.ref_d16("offset1024", run)[frame]
            share = float((d16 >= 0).mean())
            print("offset1024 frame %d d0 %d cyclic %d: valid %.4f (%.4f), largest d16 %d (%d)"
                  % (frame, d0, run.cyclic, share, (case.rows - shift) / case.rows, d16.max(), shift * 16))
            assert abs(share - (case.rows - shift) / case.rows) <= 0.02
            assert abs(int(d16.max()) - shift * 16) <= 16
            assert np.nonzero(d16 >= 0)[0].min() >= d0
            assert shift * 16 + 16 < 32767 and (d0 + 63) * 16 + 8 < 32767        # (the int16 map holds every value)


def test_offset_beyond_has_no_reachable_pixel():
    for run in cases.BY_NAME["offset_beyond"].runs:
        P1, P2, _, _, d0 = run.opts
        S = cases.ref_S("offset_beyond", d0, P1, P2, run.cyclic)
        assert (cases.ref_d16("offset_beyond", run) == -1).all()
        assert (S == 4 * 64).all()        # (every cost is 64, so every path carries 64)


@pytest.mark.parametrize("name", ["wide700", "wide16384"])
def test_the_wide_cases_see_the_seam_and_only_the_seam(name):
    case = cases.BY_NAME[name]
    differ = cases.ref_census(name, False) != cases.ref_census(name, True)
    want = [0, 1, 2, case.cols - 3, case.cols - 2, case.cols - 1]
    assert np.unique(np.nonzero(differ)[-1]).tolist() == want
    for run in case.runs:
        if not run.cyclic:
            P1, P2, _, _, d0 = run.opts
            assert not np.array_equal(cases.ref_S(name, d0, P1, P2, False), cases.ref_S(name, d0, P1, P2, True)), run
    assert cases.ref_census(name, True).shape[0] == 2 * len(case.frames) >= 4


def test_many_small_frames_are_all_different():
    case = cases.BY_NAME["many_small"]
    assert len(case.frames) * case.rows * case.cols > 64 * 4 and 64 > 4 * case.rows * case.cols
    for run in case.runs:
        d16 = cases.ref_d16("many_small", run)
        assert len({f.tobytes() for f in d16}) == len(d16) == 130, run
        assert sum(bool((f >= 0).any()) for f in d16) >= 65, run
    top, _ = cases.frames("many_single")
    assert top.shape == (300, 1, 1) and len(np.unique(top)) > 100


def test_every_case_has_frames_of_different_content():
    for case in cases.CASES:
        top, bot = cases.frames(case.name)
        assert top.shape == bot.shape == (len(case.frames), case.rows, case.cols) and len(top) >= 2
        assert not np.array_equal(top[0], top[1]) or not np.array_equal(bot[0], bot[1]), case.name
        assert len(case.runs) == len(set(case.runs)) >= 1


def test_working_finds_its_planted_shift():
    """Measured: 0.9651 of the unmasked pixels of frame 0 are valid within one row of 5 rows."""
    run = cases.BY_NAME["working"].runs[0]
    assert run.masked and run.cyclic
    d16 = cases.ref_d16("working", run)[0]
    inside = cases.mask("working") != 0
    good = (d16 >= 0) & (np.abs(d16.astype(np.int32) - 80) <= 16)
    print("working: %.4f of the unmasked pixels are valid with |d16 - 80| <= 16" % good[inside].mean())
    assert good[inside].mean() > 0.5 and (d16[~inside] == -1).all()


# ---- the new speckle families --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(3, 1000), (146, 1440)], ids=lambda s: "%dx%d" % s)
def test_new_speckle_families_equal_scipys_label(shape):
    """As tests/test_speckle_reference.py does for the other families: max_diff 32767 joins every pair of valid neighbours, and
    the components are scipy.ndimage.label's (4-connected), for the cyclic form after merging across the seam."""
    from scipy import ndimage
    rows, cols = shape
    names, d = speckle_long_cases.new_frames(*shape)
    for name, f in zip(names, d):
        for cyclic in (False, True):
            lab = refspeckle.labels_of(f, 32767, cyclic)
            theirs, count = ndimage.label(f >= 0, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
            if cyclic:
                alias = np.arange(count + 1)
                for r in range(rows):
                    a, b = theirs[r, 0], theirs[r, cols - 1]
                    if a and b:
                        lo, hi = sorted((alias[a], alias[b]))
                        alias[alias == hi] = lo
                theirs = alias[theirs]
            valid = f >= 0
            assert np.array_equal(lab != refspeckle.NONE, valid), name
            pairs = np.unique(np.stack([lab[valid].astype(np.int64), theirs[valid]]), axis=1)
            assert len(np.unique(pairs[0])) == pairs.shape[1] == len(np.unique(pairs[1])), (name, cyclic)
            # the label is the component's smallest row-major index
            first = np.full(int(theirs.max()) + 1, lab.size, np.int64)
            np.minimum.at(first, theirs[valid], np.nonzero(valid.reshape(-1))[0])
            assert np.array_equal(lab[valid], first[theirs[valid]]), (name, cyclic)


@pytest.mark.parametrize("shape", [(3, 1000), (146, 1440)], ids=lambda s: "%dx%d" % s)
def test_the_new_speckle_families_are_what_their_names_say(shape):
    rows, cols = shape
    names, d = speckle_long_cases.new_frames(*shape)
    f = {n: x.astype(np.int32) for n, x in zip(names, d)}
    edges = np.array(speckle_long_cases.ROUND_EDGES)
    # round_edges: the nine breaks in every row (the odd rows one column later), none elsewhere.  No run is longer than 256
    # up to the last break; what follows it is the rest of the row (230 columns at 1000, 670 at 1440)
    assert (f["round_edges"] >= 0).all()
    for r in range(rows):
        brk = np.nonzero(np.abs(np.diff(f["round_edges"][r])) > 16)[0] + 1
        assert np.array_equal(brk, edges + (r & 1)), r
        assert np.diff(np.concatenate([[0], brk])).max() <= 256
    if cols - edges[-1] <= 256:
        for r in range(rows):
            brk = np.nonzero(np.abs(np.diff(f["round_edges"][r])) > 16)[0] + 1
            assert np.diff(np.concatenate([[0], brk, [cols]])).max() <= 256
    assert np.abs(np.diff(f["round_edges"], axis=0)).max() == 17       # some vertical pairs beside a break are not joined
    # long_runs: no break on the even rows, one on the odd rows, in the last round
    assert (f["long_runs"] >= 0).all()
    for r in range(rows):
        brk = np.nonzero(np.abs(np.diff(f["long_runs"][r])) > 16)[0] + 1
        assert len(brk) == (r & 1) and (len(brk) == 0 or brk[0] >= (cols - 1) // 256 * 256 >= 768)
    # spiral: one component, one pixel wide (no 2 x 2 block of valid pixels), longer than a third of the frame
    valid = f["spiral"] >= 0
    for cyclic in (False, True):
        lab = refspeckle.labels_of(d[2], 16, cyclic)
        assert (lab[valid] == 0).all() and (lab[~valid] == refspeckle.NONE).all()
    assert not (valid[:-1, :-1] & valid[1:, :-1] & valid[:-1, 1:] & valid[1:, 1:]).any()
    assert valid.sum() > rows * cols // 3
    inner = valid[1:-1, 1:-1]       # a corridor: every pixel but the two ends has exactly two neighbours
    around = valid[:-2, 1:-1].astype(int) + valid[2:, 1:-1] + valid[1:-1, :-2] + valid[1:-1, 2:]
    assert (around[inner] <= 2).all()


def test_the_working_size_holds_a_component_above_65535():
    batches = speckle_long_cases.batches(146, 1440)
    names, d = [b for b in batches if b[0][0] == "constant"][0]
    lab = refspeckle.labels_of(d[0], 16, False)
    assert np.unique(lab, return_counts=True)[1].max() == 146 * 1440 > 65535
    many_names, many = speckle_long_cases.many()
    assert many.shape == speckle_long_cases.MANY[2:] + speckle_long_cases.MANY[:2] and len(set(many_names)) == 15
