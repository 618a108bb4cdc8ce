"""The candidate limit of the goodFeaturesToTrack oracle (oracle.gft_select(..., cand_cap=N)): only the N strongest
candidates -- descending response, higher address first among equal ones -- enter the greedy pass.  This is the rule of
the GPU selection, which sorts 4096 or 16384 candidates per problem; the reference here is a plain numpy restatement of
goodFeaturesToTrack written below, not the C oracle."""
import numpy as np
import pytest

import oracle


def gft_numpy(eig, mask, quality, min_distance, max_corners=0, cand_cap=0):
    """goodFeaturesToTrack restated: threshold at quality * max over the mask, 3x3 maxima of the thresholded map among
    the interior pixels of the mask, sorted by (response descending, address descending), cut to cand_cap, then the greedy
    pass with the float rule dx*dx + dy*dy < md*md.  -> (kp [n,2] float32, number of candidates before the cut)."""
    rows, cols = eig.shape
    mask = mask.astype(bool)
    if not mask.any():
        return np.zeros((0, 2), np.float32), 0
    thr = np.float32(np.float64(eig[mask].max()) * quality)
    t = np.where(eig > thr, eig, np.float32(0))
    dil = t.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            dil[1:-1, 1:-1] = np.maximum(dil[1:-1, 1:-1], t[1 + dy:rows - 1 + dy, 1 + dx:cols - 1 + dx])
    is_cand = (t != 0) & (t == dil) & mask
    is_cand[0], is_cand[-1], is_cand[:, 0], is_cand[:, -1] = False, False, False, False
    idx = np.flatnonzero(is_cand)
    n_cand = len(idx)
    v = eig.ravel()[idx]
    order = np.lexsort((-idx, -v.astype(np.float64)))        # last key first: response descending, then address descending
    idx = idx[order]
    if cand_cap > 0:
        idx = idx[:cand_cap]
    md2 = np.float32(min_distance * min_distance)
    acc = []
    for i in idx:
        x, y = np.float32(i % cols), np.float32(i // cols)
        if min_distance >= 1 and acc:
            a = np.asarray(acc, np.float32)
            dx, dy = x - a[:, 0], y - a[:, 1]
            if (dx * dx + dy * dy < md2).any():
                continue
        acc.append((x, y))
        if max_corners > 0 and len(acc) == max_corners:
            break
    return np.asarray(acc, np.float32).reshape(-1, 2), n_cand


@pytest.fixture(scope="module")
def noise():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (96, 160), dtype=np.uint8)
    return oracle.min_eigen(img), np.ones((96, 160), np.uint32)


@pytest.mark.parametrize("min_distance", [0.0, 5.0, 9.0])
def test_cap_below_the_candidate_count_equals_the_restatement_and_is_a_prefix(noise, min_distance):
    eig, bits = noise
    want_full, n_cand = gft_numpy(eig, bits, 1e-4, min_distance)
    assert 600 < n_cand < 2000                                # (about 1000 candidates: 300 is well below)
    want, _ = gft_numpy(eig, bits, 1e-4, min_distance, cand_cap=300)
    got, _, count = oracle.gft_select(eig, bits, 0, 1e-4, min_distance, 0, cand_cap=300, with_count=True)
    full, _, count_full = oracle.gft_select(eig, bits, 0, 1e-4, min_distance, 0, with_count=True)
    assert count == count_full == n_cand                      # the count is the one before the cut
    assert np.array_equal(got, want) and np.array_equal(full, want_full)
    assert 0 < len(got) < len(full) and np.array_equal(full[: len(got)], got)      # a prefix, and the cut shows
    if min_distance < 1:
        assert len(got) == 300 and len(full) == n_cand
    # with a budget reached inside the cut the result is the unlimited one
    b, _ = oracle.gft_select(eig, bits, 0, 1e-4, min_distance, 40, cand_cap=300)
    assert np.array_equal(b, full[:40]) and np.array_equal(b, gft_numpy(eig, bits, 1e-4, min_distance, 40, 300)[0])


@pytest.mark.parametrize("min_distance", [0.0, 5.0])
def test_cap_at_or_above_the_candidate_count_changes_nothing(noise, min_distance):
    eig, bits = noise
    full, maxv, n_cand = oracle.gft_select(eig, bits, 0, 1e-4, min_distance, 0, with_count=True)
    assert n_cand == gft_numpy(eig, bits, 1e-4, min_distance)[1]
    for cand_cap in (n_cand, n_cand + 1, 4096, 0, -1):
        got, maxv2, count = oracle.gft_select(eig, bits, 0, 1e-4, min_distance, 0, cand_cap=cand_cap, with_count=True)
        assert np.array_equal(got, full) and maxv2 == maxv and count == n_cand, cand_cap
    one_less, _ = oracle.gft_select(eig, bits, 0, 1e-4, 0.0, 0, cand_cap=n_cand - 1)
    all_of_them, _ = oracle.gft_select(eig, bits, 0, 1e-4, 0.0, 0)
    assert np.array_equal(one_less, all_of_them[:-1])         # the cut drops the weakest candidate, nothing else


def test_cut_inside_a_run_of_tied_responses_keeps_the_higher_addresses():
    """A periodic tile gives a plateau of equal responses on which every pixel is a candidate; a cut inside it keeps the
    highest addresses (the sort order among equal responses), and a masked problem counts its own candidates only."""
    tile = np.array([[255, 0, 0, 0], [255, 0, 0, 0], [255, 255, 0, 255]], dtype=np.uint8)
    img = np.tile(tile, (14, 12))[:40, :48]
    eig = oracle.min_eigen(img)
    bits = np.ones(img.shape, np.uint32)
    bits[:, :10] = 2
    plateau = eig[20, 20]
    assert plateau > 0 and (eig[5:35, 15:43] == plateau).all()
    for md in (0.0, 3.0):
        want, n_cand = gft_numpy(eig, bits & 1, 0.01, md, cand_cap=200)
        got, _, count = oracle.gft_select(eig, bits, 0, 0.01, md, 0, cand_cap=200, with_count=True)
        assert count == n_cand > 1000 and np.array_equal(got, want)
        full, _ = oracle.gft_select(eig, bits, 0, 0.01, md, 0)
        assert len(got) < len(full) and np.array_equal(full[: len(got)], got)
    cut, _ = oracle.gft_select(eig, bits, 0, 0.01, 0.0, 0, cand_cap=200)
    on_plateau = eig[cut[:, 1].astype(int), cut[:, 0].astype(int)] == plateau
    addr = (cut[:, 1] * img.shape[1] + cut[:, 0])[on_plateau]
    all_plateau = np.flatnonzero((eig == plateau) & (bits & 1).astype(bool))
    interior = [a for a in all_plateau if 0 < a // 48 < 39 and 0 < a % 48 < 47]
    assert on_plateau.sum() > 100 and np.array_equal(addr, np.sort(interior)[::-1][: on_plateau.sum()])


def test_flow_passes_the_cap_its_capacity_implies():
    assert oracle.gft_cand_cap(320) == oracle.gft_cand_cap(1024) == 4096
    assert oracle.gft_cand_cap(1025) == oracle.gft_cand_cap(2048) == 16384
