"""sosvo_sort_matches as a stable counting sort over the 12-bit distance field, with the rank sort
kept for problems of at most a wave: ctx.sort_matches against oracle.sort_matches, order[:n] exactly, order[n:] untouched.

Every n of N_LIST runs eight key sets as the eight problems of one launch, once with q_stride = n rounded up to a multiple of
four (the smallest stride the entry's LDS layout distinguishes) and once with a larger, odd stride.  The n list holds both
sides of the threshold between the two forms (kSortRankMaxN, read from csrc/match.hip), of the 64-query chunks of the
placement walk, of the 256 threads of the load loop, and one n beyond 4096 (more queries than bins)."""
import os
import re

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
SENTINEL = -7
N_LIST = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4097]


def _key(dist, idx):
    return ((np.asarray(dist, np.uint64) << 20) | (np.asarray(idx, np.uint64) & 0xFFFFF)).astype(np.uint32)


def _with_none_runs(rng, keys):
    """NONE mixed in at random, and in runs of 64 .. 130 from random starts."""
    keys = keys.copy()
    n = len(keys)
    keys[rng.random(n) < 0.2] = NONE
    pos = 0
    while pos < n:
        pos += int(rng.integers(0, 200))
        run = int(rng.integers(64, 131))
        keys[pos:pos + run] = NONE
        pos += run + 1
    return keys


def key_sets(rng, n):
    """The eight key sets of the issue for one n, each [n] u32."""
    idx = rng.integers(0, 1 << 20, n)
    i = np.arange(n)
    sets = []
    sets.append(_key(rng.integers(0, 257, n), idx))                                   # random Hamming distances
    sets.append(_key(np.full(n, 93), idx))                                            # one distance
    sets.append(_key(np.where(i % 2 == 0, 40, 7), idx))                               # two distances alternating
    span = min(max(n - 1, 0), 0xFFE)
    sets.append(_key(((n - 1 - i) * span) // max(n - 1, 1), idx))                     # descending (strictly up to 4095 keys)
    sets.append(np.full(n, NONE, np.uint32))                                          # all NONE
    sets.append(_with_none_runs(rng, _key(rng.integers(0, 257, n), idx)))             # NONE at random and in runs
    full = _key(rng.choice([0, 257, 0x7FF, 0xFFE, 0xFFF], n), idx)                    # the whole 12-bit range
    full[rng.random(n) < 0.1] = NONE
    sets.append(full)
    one = np.full(n, NONE, np.uint32)                                                 # one key that is not NONE
    if n:
        one[int(rng.integers(0, n))] = _key(17, 5)
    sets.append(one)
    return sets


def _run(ctx, problems, q_stride, nq=None, q_slot=None):
    """problems: list of [n_p] u32 key arrays -> checks every problem of one launch; returns order."""
    P = len(problems)
    keys = np.full((P, q_stride, 1), 0x12345678, np.uint32)          # (rows past n hold keys that must not be read as such)
    for p, k in enumerate(problems):
        keys[p, :len(k), 0] = k
    if nq is None:
        nq = np.array([len(k) for k in problems], np.int32)
    dev = ctx.device
    order = torch.full((P, q_stride), SENTINEL, dtype=torch.int32, device=dev)
    t_slot = None if q_slot is None else torch.from_numpy(np.asarray(q_slot, np.int32)).to(dev)
    ctx.sort_matches(torch.from_numpy(keys).to(dev), torch.from_numpy(np.asarray(nq, np.int32)).to(dev), order=order, q_slot=t_slot)
    ctx.synchronize()
    order = order.cpu().numpy()
    for p, k in enumerate(problems):
        n = len(k)
        want = oracle.sort_matches(k) if n else np.zeros(0, np.int32)
        assert np.array_equal(order[p, :n], want), "problem %d of %d, n %d, q_stride %d" % (p, P, n, q_stride)
        assert (order[p, n:] == SENTINEL).all(), "problem %d, n %d: a row past n was written" % (p, n)
    return order


def test_n_list_holds_both_sides_of_the_threshold():
    src = open(os.path.join(ROOT, "vo_single_camera_sos_amd", "csrc", "match.hip")).read()
    t = int(re.search(r"constexpr int kSortRankMaxN = (\d+);", src).group(1))
    assert t in N_LIST and t + 1 in N_LIST


@pytest.mark.parametrize("n", N_LIST)
def test_key_sets_at_two_strides(ctx, n):
    rng = np.random.default_rng(1000 + n)
    sets = key_sets(rng, n)
    tight = max(4, (n + 3) & ~3)
    _run(ctx, sets, tight)
    _run(ctx, sets, tight + 37)


def test_forty_problems_through_repeated_slots(ctx):
    """One launch of 40 problems of different n, some 0, on both sides of the threshold: nq has 12 entries, q_slot repeats them."""
    rng = np.random.default_rng(40)
    q_stride = 700
    nq = np.array([0, 1, 64, 65, 200, 700, 63, 0, 333, 129, 512, 650], np.int32)
    q_slot = rng.integers(0, len(nq), 40).astype(np.int32)
    q_slot[:12] = np.arange(12)
    problems = []
    for p in range(40):
        n = int(nq[q_slot[p]])
        problems.append(key_sets(rng, n)[(0, 5, 6, 2)[p % 4]])
    _run(ctx, problems, q_stride, nq=nq, q_slot=q_slot)


def test_nq_larger_than_the_stride_is_clamped(ctx):
    rng = np.random.default_rng(41)
    for q_stride in (60, 300):
        problems = [key_sets(rng, q_stride)[s] for s in (0, 5, 6)]
        _run(ctx, problems, q_stride, nq=np.array([q_stride + 1, 5000, 1 << 30], np.int32))


def test_the_largest_stride(ctx):
    """q_stride = 16384, the entry's limit: the fields of 16384 queries and the bins fill the workgroup's LDS."""
    rng = np.random.default_rng(42)
    n = 16384
    _run(ctx, [key_sets(rng, n)[0], key_sets(rng, n)[6], key_sets(rng, 100)[0]], n)
