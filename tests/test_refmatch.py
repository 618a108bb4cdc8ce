"""CPU: the one definition of a match under the matcher options (tests/refmatch.py) against evaluations that do not share
its code -- the oracle's matcher, compositions of oracle calls, plain loops, hand-built rows.  Problems come from
matching_scenes.descriptor_scene (planted re-observations, duplicate rows: ties occur); sizes 0, 1, 2 and both sides of the
matcher's 32-query / 128-train tile edges, and a few random ones up to 140."""
import numpy as np
import pytest

import oracle
import refflow
from matching_scenes import descriptor_scene
from refmatch import IDX, NONE, Matching, gate_matrix, two_smallest_keys

SIZES = (0, 1, 2, 33, 129)
GATE = (1.0, 2.5)


def _problems():
    rng = np.random.default_rng(811)
    shapes = [(a, b) for a in SIZES for b in SIZES] + [tuple(rng.integers(1, 141, 2)) for _ in range(6)]
    for nq, nt in shapes:
        desc, pos = descriptor_scene(rng, 2, 144, np.array([nt, nq]))
        yield desc[1, :nq], desc[0, :nt], pos[1, :nq], pos[0, :nt]


PROBLEMS = list(_problems())


def _same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


def test_the_problems_have_ties():
    tied = 0
    for q, t, _, _ in PROBLEMS:
        if len(q) and len(t) > 1:
            two = oracle.match_hamming(q, t, k=2).reshape(-1, 2)
            tied += int(((two[:, 0] >> 20) == (two[:, 1] >> 20)).sum())
    assert tied > 20


def test_without_options_it_is_refflows_matcher():
    for q, t, qp, tp in PROBLEMS:
        assert _same(Matching()(q, t, qp, tp, GATE), refflow.match_sorted(q, t)), (len(q), len(t))


def test_two_smallest_keys_are_the_oracles_two_nearest():
    for q, t, _, _ in PROBLEMS:
        if len(q) and len(t):
            k1, k2 = two_smallest_keys(q, t)
            two = oracle.match_hamming(q, t, k=2).reshape(len(q), -1)
            assert np.array_equal(k1, two[:, 0]), (len(q), len(t))
            assert np.array_equal(k2, two[:, 1] if len(t) > 1 else np.full(len(q), NONE, np.uint32)), (len(q), len(t))


def test_mutual_is_two_oracle_searches_and_the_index_test():
    kept = rejected = 0
    for q, t, qp, tp in PROBLEMS:
        got = Matching(mutual=True)(q, t, qp, tp, GATE)
        if len(q) == 0 or len(t) == 0:
            assert all(len(a) == 0 for a in got)
            continue
        fwd = oracle.match_hamming(q, t, k=1)[:, 0]
        rev = oracle.match_hamming(t, q, k=1)[:, 0]
        idx = np.nonzero((rev[fwd & IDX] & IDX) == np.arange(len(q)))[0]
        order = oracle.sort_matches(fwd[idx])          # stable: ties keep query order
        want = (idx[order].astype(np.int64), (fwd[idx][order] & IDX).astype(np.int64), (fwd[idx][order] >> 20).astype(np.int64))
        assert _same(got, want), (len(q), len(t))
        kept, rejected = kept + len(idx), rejected + len(q) - len(idx)
    assert kept > 100 and rejected > 100


def test_gated_with_both_gate_sides_off_and_no_cap_is_the_plain_search():
    for q, t, qp, tp in PROBLEMS:
        for mutual in (False, True):
            assert _same(Matching(gated=True, mutual=mutual)(q, t, qp, tp, (-1.0, -1.0)), Matching(mutual=mutual)(q, t, qp, tp, None))


@pytest.mark.parametrize("cap", [None, 80])
def test_gated_matches_pass_the_gate_and_no_admissible_train_is_nearer(cap):
    """In plain loops: every kept match passes oracle.pixel_gates (and the cap), no admissible train of its query has a
    smaller key, and a query without a match has no admissible train within the cap."""
    kept = dropped = 0
    for q, t, qp, tp in PROBLEMS:
        qi, ti, dist = Matching(gated=True, cap=cap)(q, t, qp, tp, GATE)
        assert len(set(qi.tolist())) == len(qi)
        match = dict(zip(qi.tolist(), zip(ti.tolist(), dist.tolist())))
        rows_q, rows_t = [int.from_bytes(r.tobytes(), "little") for r in q], [int.from_bytes(r.tobytes(), "little") for r in t]
        for i in range(len(q)):
            best = None
            passes = oracle.pixel_gates(tp.astype(np.float64), np.repeat(qp[i:i + 1].astype(np.float64), len(t), 0), *GATE) if len(t) else []
            for j in range(len(t)):
                key = (bin(rows_q[i] ^ rows_t[j]).count("1"), j)
                if passes[j] and (best is None or key < best):
                    best = key
            if best is not None and best[0] > (256 if cap is None else cap):
                best = None
            assert match.get(i) == (None if best is None else (best[1], best[0])), (len(q), len(t), i)
            kept, dropped = kept + (best is not None), dropped + (best is None)
    assert kept > 100 and dropped > 100


def test_the_reversed_gate_is_the_gate_with_the_roles_swapped():
    for q, t, qp, tp in PROBLEMS:
        if len(q) and len(t):
            assert np.array_equal(gate_matrix(tp, qp, *GATE, reverse=True), gate_matrix(qp, tp, *GATE).T)


def _bits(d):
    row = np.zeros(32, np.uint8)
    for b in range(d):
        row[b >> 3] |= np.uint8(1 << (b & 7))
    return row


def test_ratio_63_on_hand_built_rows():
    """One zero query per row against two trains with d1 < d2 set bits: kept <=> 64 * d1 < 63 * d2."""
    pairs = [(0, 1), (1, 2), (62, 63), (63, 64), (63, 65), (100, 101), (100, 102), (126, 128), (127, 129), (200, 204), (5, 200)]
    q = np.zeros((1, 32), np.uint8)
    pos = np.zeros((2, 2), np.float32)
    for d1, d2 in pairs:
        t = np.stack([_bits(d2), _bits(d1)])
        qi, ti, dist = Matching(ratio=63)(q, t, pos[:1], pos, None)
        if 64 * d1 < 63 * d2:
            assert (qi.tolist(), ti.tolist(), dist.tolist()) == ([0], [1], [d1]), (d1, d2)
        else:
            assert len(qi) == 0, (d1, d2)
    assert {64 * a < 63 * b for a, b in pairs} == {True, False}
