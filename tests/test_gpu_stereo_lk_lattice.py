"""GPU: sosvo_refine_stereo_lk against tests/refstereolk.py bit for bit on the cases of tests/lk_lattice_cases.py (whose content
tests/test_lk_lattice_reference.py vouches for on the CPU):

- half 3, 5, 6 and 9 on the scene of tests/test_gpu_stereo_lk.py (2 frames, 3 masks, cap 16): both sides of the switch between
  the 16-lane and the whole-wave mapping, and windows whose element counts are no multiple of the group;
- the gather across its rounds of 256 rows: cap 600, bottom counts (600, 257, 256, 0), about a third of the rows scattered
  among dropped keys, top rows at and beyond n_top, pairs the pre-gate skips and non-finite keypoints, so that every round
  compacts another number of rows onto the running count -- and the tracker behind it takes later rounds of its keypoint loop
  (363 gathered rows: two rounds at half 4, six at half 6).

kp_bot (uint32 bit patterns) and the status are compared over the whole buffers; the status starts as 0xA5 and the rows of
kp_bot beyond n_bot as -123.25, and both must hold there; what the stage only reads is compared with what it was handed."""
import numpy as np
import pytest
import torch

import lk_lattice_cases as cases

pytestmark = pytest.mark.gpu


def _dev(ctx, a):
    return torch.from_numpy(np.array(a)).to(ctx.device)       # (a copy: the cases' arrays are read-only)


def _compare(ctx, case):
    t = {k: _dev(ctx, getattr(case, k)) for k in ("gray", "kp_top", "n_top", "kp_bot", "n_bot", "keys")}
    status = torch.full((case.nprob, case.cap), cases.ST_SENTINEL, dtype=torch.uint8, device=ctx.device)
    ctx.refine_stereo_lk(t["gray"], t["kp_top"], t["n_top"], t["kp_bot"], t["n_bot"], t["keys"], case.nmask, case.min_disp, case.max_hdiff,
                         stereo_lk=case.opts, status=status)
    ctx.synchronize()
    want = cases.stereo_reference(case)
    for g, w, name in ((t["kp_bot"].cpu().numpy().view(np.uint32), want[0].view(np.uint32), "kp_bot"),
                       (status.cpu().numpy(), want[1], "status")):
        bad = np.argwhere(g != w)
        assert bad.size == 0, (case, name, len(bad), [(tuple(b), g[tuple(b)], w[tuple(b)]) for b in bad[:4]])
    for p, nb in enumerate(case.n_bot):                      # (the reference leaves these rows alone: stated once more)
        assert (want[0][p, nb:] == cases.SENTINEL).all() and (want[1][p, nb:] == cases.ST_SENTINEL).all()
    for k in ("kp_top", "n_top", "n_bot", "keys", "gray"):
        assert np.array_equal(t[k].cpu().numpy().view(np.uint8), getattr(case, k).view(np.uint8)), k


@pytest.mark.parametrize("half", cases.STEREO_HALVES)
def test_stage_equals_the_reference_at_the_switch(ctx, half):
    _compare(ctx, cases.stereo_case(half))


@pytest.mark.parametrize("half", cases.GATHER_HALVES)
def test_gather_across_rounds_equals_the_reference(ctx, half):
    _compare(ctx, cases.gather_case(half))
