"""The definition of a match under the matcher options (include/sosvo.h: the gated search, the ratio rule, the cap, the
mutual-consistency filter), written once in numpy on top of the oracle (test infrastructure, like refflow.py; also read by
scripts/fuzz_parity.py).  A Matching is the test-side twin of one matching step's share of _lib.MatchOptions; refflow's
flow functions take one as their `matching` argument."""
from collections import namedtuple

import numpy as np

import oracle

IDX, NONE = 0xFFFFF, 0xFFFFFFFF
POPCOUNT = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint32)


def distances(q, t):
    """[nq, nt] Hamming distances."""
    return POPCOUNT[q[:, None, :] ^ t[None, :, :]].sum(-1, dtype=np.uint32)


def gate_matrix(q_pos, t_pos, min_dv, max_du, reverse=False):
    """gate(i, j) [nq, nt]: oracle.pixel_gates(train, query) on doubles converted from the float32 positions; a reversed
    problem evaluates the same gate with the roles swapped (v_q - v_t >= min_dv)."""
    nq, nt = len(q_pos), len(t_pos)
    qp = np.repeat(q_pos.astype(np.float64)[:, None, :], nt, 1).reshape(-1, 2)
    tp = np.repeat(t_pos.astype(np.float64)[None, :, :], nq, 0).reshape(-1, 2)
    ok = oracle.pixel_gates(qp, tp, min_dv, max_du) if reverse else oracle.pixel_gates(tp, qp, min_dv, max_du)
    return ok.reshape(nq, nt)


def two_smallest_keys(q, t, admissible=None):
    """(k1, k2): the two smallest keys (hamming << 20 | j) over the admissible trains of every query, NONE where absent."""
    nq, nt = len(q), len(t)
    keys = np.full((nq, nt + 2), NONE, np.uint32)
    if nq and nt:
        k = (distances(q, t) << 20) | np.arange(nt, dtype=np.uint32)[None, :]
        keys[:, :nt] = k if admissible is None else np.where(admissible, k, np.uint32(NONE))
    keys.sort(axis=1)
    return keys[:, 0].copy(), keys[:, 1].copy()


def capped(k1, cap=None):
    """The 1-NN keys with the winners beyond the cap dropped (NONE >> 20 is 4095: NONE stays NONE)."""
    return np.where((k1 >> 20) > (256 if cap is None else cap), np.uint32(NONE), k1).astype(np.uint32)


def ratio_rule(k1, k2, r, gated, cap=256):
    """keep(i) <=> 64 * d1 < r * d2; no runner-up: dropped in the plain form, kept in the gated one; then the cap."""
    d1, d2 = (k1 >> 20).astype(np.int64), (k2 >> 20).astype(np.int64)
    keep = np.where(k2 == NONE, bool(gated), 64 * d1 < r * d2) & (k1 != NONE) & (d1 <= cap)
    return np.where(keep, k1, np.uint32(NONE)).astype(np.uint32)


class Matching(namedtuple("Matching", "gated cap mutual ratio", defaults=(False, None, False, 0))):
    """One matching step's options.  gated: search only among the trains that pass the step's pixel gate, with cap as the
    largest distance kept (256 without one, and whenever the step is not gated); mutual: the cross-check; ratio: Lowe's rule
    in 64ths, 0 for none."""
    __slots__ = ()

    def keys(self, qd, td, qp, tp, gate, reverse=False):
        """The keys [nq] before the mutual filter, NONE where dropped.  gate = (min_dv, max_du), read only when gated.
        reverse: a role-swapped problem -- the gate with the roles swapped, the cap, and WITHOUT the ratio rule."""
        if len(qd) == 0 or len(td) == 0:
            return np.full(len(qd), NONE, np.uint32)
        cap = self.cap if self.gated and self.cap is not None else 256
        k1, k2 = two_smallest_keys(qd, td, gate_matrix(qp, tp, gate[0], gate[1], reverse) if self.gated else None)
        return ratio_rule(k1, k2, self.ratio, self.gated, cap) if self.ratio and not reverse else capped(k1, cap)

    def kept(self, qd, td, qp, tp, gate):
        """The keys [nq] after the mutual filter: query i keeps its train only if the role-swapped search of that train
        returns i."""
        fwd = self.keys(qd, td, qp, tp, gate)
        keep = fwd != NONE
        if self.mutual and keep.any():
            back = self.keys(td, qd, tp, qp, gate, reverse=True)[np.where(keep, fwd & IDX, 0)]
            keep &= (back != NONE) & ((back & IDX) == np.arange(len(qd)))
        return np.where(keep, fwd, np.uint32(NONE)).astype(np.uint32)

    def __call__(self, qd, td, qp, tp, gate):
        """refflow.match_sorted of one problem under the options -> (query_idx, train_idx, dist), stably sorted by
        distance; an empty side gives three empty arrays."""
        keys = self.kept(qd, td, qp, tp, gate)
        kept = np.nonzero(keys != NONE)[0]
        k = keys[kept]
        order = oracle.sort_matches(k) if len(k) else np.zeros(0, np.int64)
        return kept[order].astype(np.int64), (k[order] & IDX).astype(np.int64), (k[order] >> 20).astype(np.int64)
