"""GPU: Lowe's ratio rule fused into the matrix-core matcher (sosvo_match_hamming_ratio), stage level.

The CPU checker is the definition of include/sosvo.h written in numpy (tests/refmatch.py, two_smallest_keys / ratio_rule): the
popcount distance matrix, oracle.pixel_gates on doubles converted from the float32 positions, the two smallest packed keys over
the admissible trains, the integer rule 64 * d1 < r * d2, the cap.  keys and rivals are compared bit for bit."""
import numpy as np
import pytest
import torch

import oracle
from matching_scenes import StageProblems, descriptor_scene as _scene
from refmatch import NONE, capped, ratio_rule

pytestmark = pytest.mark.gpu

RATIOS = (1, 48, 63)
# (query count, train count) at the edges of the 32-query tiles, the 32-row blocks and the 128-train tiles
COUNTS = ((1, 1), (1, 2), (33, 2), (31, 127), (32, 128), (33, 129), (129, 257))
GROUPS = ((0, 1, 2), (3, 4, 5), (6, 0, 4))                       # three problems per call


class _Stage(StageProblems):
    """sosvo_match_hamming_ratio on the problems, the last P - n_forward of them reversed, against the definition."""

    def run(self, r, gate=None, cap=None, n_forward=None, **kw):
        pos = {} if gate is None else dict(q_pos=self.d_qp, t_pos=self.d_tp, min_dv=gate[0], max_du=gate[1], max_distance=cap)
        pos.update(self.sl)
        pos.update(kw)
        keys, rivals = self.ctx.match_hamming_ratio(self.d_qd, self.d_td, self.d_nq, self.d_nt, r, n_forward=n_forward, **pos)
        self.ctx.synchronize()
        return keys.cpu().numpy()[:, :, 0], rivals.cpu().numpy()[:, :, 0]

    def expect(self, p, r, gate, cap, n_forward):
        """(keys, rivals or None) of problem p; a reversed problem's keys are the unfiltered, capped 1-NN keys."""
        if p < n_forward:
            k1, k2 = self.smallest(p, gate, False)
            return ratio_rule(k1, k2, r, gate is not None, 256 if cap is None else cap), k2
        return capped(self.smallest(p, gate, True)[0], cap), None

    def check(self, r, gate=None, cap=None, n_forward=None):
        nf = self.P if n_forward is None else n_forward
        keys, rivals = self.run(r, gate, cap, nf)
        for p in range(self.P):
            wk, wr = self.expect(p, r, gate, cap, nf)
            assert np.array_equal(keys[p, : len(wk)], wk), ("keys", p, r, gate, cap, nf)     # (padding rows are unspecified)
            if wr is not None:
                assert np.array_equal(rivals[p, : len(wr)], wr), ("rivals", p, r, gate, cap, nf)
        return keys, rivals


FORMS = [(None, (None,)), ((1.0, 2.5), (None, 64)), ((-1.0, 2.5), (None, 64))]   # plain; gated with dv on / off, cap 256 / 64


def _edge_stage(ctx, rng, group, q_stride, t_stride):
    nq = np.array([COUNTS[g][0] for g in group])
    nt = np.array([min(COUNTS[g][1], t_stride) for g in group])
    qd, qp = _scene(rng, 3, q_stride, nq)
    td, tp = _scene(rng, 3, t_stride, nt)
    k = min(q_stride, t_stride)
    td[:, :k:2] = qd[:, :k:2]                                     # (true partners exist: same descriptor, nearby position)
    tp[:, :k:2] = qp[:, :k:2] + rng.uniform(-2.0, 4.0, qp[:, :k:2].shape).astype(np.float32)
    return _Stage(ctx, qd, td, qp, tp, nq, nt)


# ---- 1. the stage against the definition ----------------------------------------------------------------------------------
@pytest.mark.parametrize("t_stride", [288, 128], ids=["split", "unsplit"])
def test_stage_equals_the_definition_at_the_tile_edges(ctx, t_stride):
    """Three problems per call, q_stride 160; t_stride 288: the train range is split over three workgroups and the rule is
    the elementwise pass over (best, rival); t_stride 128 (counts capped to it): one workgroup walks the trains and the rule
    is fused into its epilogue.  Plain and gated forms, dv side on and off, n_forward 0 / 1 / 3, caps, r = 1 / 48 / 63."""
    rng = np.random.default_rng(4100 + t_stride)
    kept = dropped = 0
    for group in GROUPS:
        st = _edge_stage(ctx, rng, group, 160, t_stride)
        for gate, caps in FORMS:
            for cap in caps:
                for n_forward in (0, 1, 3):
                    for r in RATIOS:
                        keys, _ = st.check(r, gate, cap, n_forward)
                        if n_forward == 3 and r == 48:
                            real = np.concatenate([keys[p, : st.nq[p]] for p in range(3)])
                            kept += int((real != NONE).sum())
                            dropped += int((real == NONE).sum())
    assert kept > 100 and dropped > 100                           # (the rule decided something both ways)


def test_stage_two_tiles_per_wave(ctx):
    """q_stride 1024: the kernel form with two query tiles per wave, nq = 1000 (a partly filled last tile), nt = 300 in a
    train stride of 320 (the range is split)."""
    rng = np.random.default_rng(29)
    nq, nt = np.array([1000]), np.array([300])
    qd, qp = _scene(rng, 1, 1024, nq)
    td, tp = _scene(rng, 1, 320, nt)
    td[0, :300:3] = qd[0, :300:3]
    tp[0, :300:3] = qp[0, :300:3] + np.float32(1.25)
    st = _Stage(ctx, qd, td, qp, tp, nq, nt)
    for gate, caps in FORMS:
        for r in RATIOS:
            st.check(r, gate, caps[-1], 1)
    st.check(48, (1.0, 2.5), None, 0)
    k = st.expect(0, 48, (1.0, 2.5), None, 1)[0]
    assert (k != NONE).sum() > 50 and (k == NONE).sum() > 50


def test_stage_slot_tables_and_role_swapped_problems(ctx):
    """40 problems through slot tables over a store of 6 blocks (one empty), as the tracking calls address their frames; the
    second half are the role-swapped twins of the first, as in a cross-checked step."""
    rng = np.random.default_rng(23)
    S, counts = 288, np.array([257, 129, 128, 33, 2, 0])
    desc, pos = _scene(rng, 6, S, counts)
    n = 20
    a, b = rng.integers(0, 6, n), rng.integers(0, 6, n)
    q_slot, t_slot = np.concatenate([a, b]), np.concatenate([b, a])
    st = _Stage(ctx, desc, desc, pos, pos, counts, counts, q_slot, t_slot)
    for gate, caps in FORMS:
        for cap in caps:
            for n_forward in (0, n, 2 * n):
                st.check(48, gate, cap, n_forward)
    st.check(63, (1.0, 2.5), 80, n)
    st.check(1, None, None, n)


# ---- 2. constructed cases -------------------------------------------------------------------------------------------------
def _bits(d):
    """A descriptor with exactly d set bits."""
    row = np.zeros(32, np.uint8)
    for b in range(d):
        row[b >> 3] |= np.uint8(1 << (b & 7))
    return row


def _constructed(ctx, trains, positions=None, t_stride=160):
    """One zero query at (100, 10) against trains with the given numbers of set bits (so distance = bits)."""
    qd = np.zeros((1, 32, 32), np.uint8)
    td = np.zeros((1, t_stride, 32), np.uint8)
    qp = np.zeros((1, 32, 2), np.float32)
    tp = np.zeros((1, t_stride, 2), np.float32)
    qp[0, 0] = (100.0, 10.0)
    for j, d in enumerate(trains):
        td[0, j] = _bits(d)
        tp[0, j] = (100.0, 12.0) if positions is None else positions[j]
    return _Stage(ctx, qd, td, qp, tp, np.array([1]), np.array([len(trains)]))


@pytest.mark.parametrize("t_stride", [160, 128], ids=["split", "unsplit"])
def test_constructed_cases(ctx, t_stride):
    gate = (1.0, 2.5)
    inside, outside = (100.0, 12.0), (150.0, 12.0)

    def both(trains, r, positions=None, cap=None):
        """(plain key, gated key) of the query, each checked against the definition with its rivals."""
        st = _constructed(ctx, trains, positions, t_stride)
        plain = st.check(r)[0][0, 0] if cap is None else None
        gated = st.check(r, gate, cap)[0][0, 0]
        return plain, gated

    assert both([4, 2], 48) == ((2 << 20) | 1, (2 << 20) | 1)     # 64 * 2 = 128 < 48 * 4 = 192: kept
    assert both([3, 4], 48) == (NONE, NONE)                       # 64 * 3 = 192 < 192 is false: dropped
    assert both([1, 0], 48) == (1, 1)                             # (0, 1): kept
    assert both([0, 0], 48) == (NONE, NONE)                       # duplicates: dropped even at distance 0
    assert both([0, 0], 63) == (NONE, NONE)
    assert both([5, 5, 9], 63) == (NONE, NONE)                    # ties resolve by train index, and a tie never passes
    assert both([7], 48) == (NONE, 7 << 20)                       # no runner-up: dropped in the plain form, kept in the gated
    # the gated form with both gate sides disabled still keeps a lone train: the form decides, not the gate values
    st = _constructed(ctx, [7], None, t_stride)
    assert st.check(48, (-1.0, 0.0), None)[0][0, 0] == 7 << 20
    # a closer rival OUTSIDE the gate is ignored as runner-up ...
    plain, gated = both([3, 4, 40], 48, [inside, outside, inside])
    assert plain == NONE and gated == 3 << 20
    # ... and as winner: train 0 is nearest but outside; inside (6, 9) passes at r = 48 (384 < 432)
    plain, gated = both([1, 6, 9], 48, [outside, inside, inside])
    assert plain == 1 << 20 and gated == (6 << 20) | 1
    # a winner beyond the cap is dropped although it passes the rule; at the cap it stays
    assert both([10, 90], 48, cap=9)[1] == NONE
    assert both([10, 90], 48, cap=10)[1] == 10 << 20
    # the rule is evaluated on the uncapped runner-up: (10, 12) fails the rule, and capping 12 away must not rescue it
    assert both([10, 12], 48, cap=11)[1] == NONE


def test_reversed_rows_equal_the_entries_without_the_rule(ctx):
    """Problems p >= n_forward: the keys of sosvo_match_hamming(k = 1) / sosvo_match_hamming_gated on the same (already
    role-swapped) problem, bit for bit; and wherever a forward key is not NONE it is that 1-NN key."""
    rng = np.random.default_rng(61)
    S, counts = 288, np.array([257, 129, 200])
    desc, pos = _scene(rng, 3, S, counts)
    q_slot, t_slot = np.array([1, 2, 0, 0, 0, 1]), np.array([0, 0, 1, 1, 2, 0])
    st = _Stage(ctx, desc, desc, pos, pos, counts, counts, q_slot, t_slot)
    nf = 3
    plain1 = ctx.match_hamming(st.d_qd, st.d_td, st.d_nq, st.d_nt, k=1, **st.sl)
    gated1 = ctx.match_hamming_gated(st.d_qd, st.d_td, st.d_qp, st.d_tp, st.d_nq, st.d_nt, min_dv=1.0, max_du=2.5, max_distance=80,
                                     n_forward=nf, **st.sl)
    ctx.synchronize()
    plain1, gated1 = plain1.cpu().numpy()[:, :, 0], gated1.cpu().numpy()[:, :, 0]
    kp, _ = st.check(48, None, None, nf)
    kg, _ = st.check(48, (1.0, 2.5), 80, nf)
    for p in range(6):
        n = counts[q_slot[p]]
        for got, base in ((kp, plain1), (kg, gated1)):
            if p >= nf:
                assert np.array_equal(got[p, :n], base[p, :n])
            else:
                on = got[p, :n] != NONE
                assert on.any() and (~on).any() and np.array_equal(got[p, :n][on], base[p, :n][on])


def test_plain_form_at_48_is_the_reference_rule_on_the_2nn_keys(ctx):
    """m[0].distance < m[1].distance * 0.75 on oracle.match_hamming(k = 2) (camera_models.py:421-423, len(m) == 2)."""
    rng = np.random.default_rng(67)
    counts = np.array([300, 257])
    qd, qp = _scene(rng, 2, 320, counts)
    td, tp = _scene(rng, 2, 320, counts[::-1].copy())
    for lo, hi in ((0, 60), (100, 160)):                          # re-observed queries: a few flipped bits against ~128 elsewhere
        flip = (np.uint8(1) << rng.integers(0, 8, (2, hi - lo, 32)).astype(np.uint8)) * (rng.integers(0, 32, (2, hi - lo, 32)) == 0)
        td[:, lo:hi] = qd[:, lo:hi] ^ flip.astype(np.uint8)
    st = _Stage(ctx, qd, td, qp, tp, counts, counts[::-1].copy())
    keys, _ = st.check(48)
    for p in range(2):
        two = oracle.match_hamming(qd[p, : counts[p]], td[p, : st.nt[p]], k=2).reshape(-1, 2)
        d1, d2 = (two[:, 0] >> 20).astype(np.float64), (two[:, 1] >> 20).astype(np.float64)
        keep = (two[:, 1] != NONE) & (d1 < d2 * 0.75)
        assert 20 < keep.sum() < len(keep)
        assert np.array_equal(keys[p, : counts[p]] != NONE, keep)
        assert np.array_equal(keys[p, : counts[p]][keep], two[keep, 0])


def test_results_do_not_depend_on_scratch_or_on_the_output_buffers_before_the_call(ctx):
    rng = np.random.default_rng(71)
    st = _edge_stage(ctx, rng, (6, 5, 4), 160, 288)
    out = []
    for byte in (0x00, 0xA5):
        ctx.debug_fill_scratch(byte)
        keys = torch.full((3, 160, 4), byte, dtype=torch.uint8, device=ctx.device).view(torch.uint32)
        rivals = keys.clone()
        for gate in (None, (1.0, 2.5)):
            k, r = st.run(48, gate, None, 3, keys=keys, rivals=rivals)
            out.append([np.concatenate([a[p, : st.nq[p]] for p in range(3)]) for a in (k, r)])
    for a, b in zip(out[:2], out[2:]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_results_do_not_depend_on_the_train_split(ctx):
    """SOSVO_HINT_MATCH_UNSPLIT: the same launch without the split (rule fused into the epilogue) gives the bits of the split
    one (atomic merge on two words, then the elementwise pass) -- keys and rivals, plain and gated, with reversed rows."""
    rng = np.random.default_rng(79)
    st = _edge_stage(ctx, rng, (6, 5, 3), 160, 288)
    split = [st.check(48, gate, cap, 2) for gate, cap in ((None, None), ((1.0, 2.5), 64))]
    ctx.set_hint_match_unsplit(True)
    try:
        whole = [st.check(48, gate, cap, 2) for gate, cap in ((None, None), ((1.0, 2.5), 64))]
    finally:
        ctx.set_hint_match_unsplit(False)
    for (ka, ra), (kb, rb) in zip(split, whole):
        for p in range(3):
            n = st.nq[p]
            assert np.array_equal(ka[p, :n], kb[p, :n])
            if p < 2:
                assert np.array_equal(ra[p, :n], rb[p, :n])


def test_stage_refuses_bad_arguments(ctx):
    from vo_single_camera_sos_amd._lib import SosvoError
    rng = np.random.default_rng(73)
    st = _edge_stage(ctx, rng, (0, 1, 2), 160, 128)
    for bad in (0, 64, -1):
        with pytest.raises(SosvoError, match="sosvo_match_hamming_ratio"):
            st.run(bad)
    with pytest.raises(SosvoError):
        ctx.match_hamming_ratio(st.d_qd, st.d_td, st.d_nq, st.d_nt, 48, q_pos=st.d_qp)       # exactly one position array
    with pytest.raises(SosvoError, match="n_forward"):
        st.run(48, None, None, 4)
    with pytest.raises(SosvoError, match="max_distance"):
        st.run(48, (1.0, 2.5), 257)
