"""GPU: gated matching -- the 1-NN search among the trains that pass the pixel gates (sosvo_match_hamming_gated) -- through
every layer: the stage entry, FeatureMatcher.match_gated, the pair pipelines and one-call batches, the sequence engines
behind run_VO / run_VO_many, RGB-D, and the subset relations the definition implies.

The CPU checker is the definition itself, composed of oracle calls (tests/refmatch.py): oracle.pixel_gates on the float32
positions converted to double, a numpy min over popcounts, oracle.sort_matches.  refflow's flow functions take it as their
matcher (matching_scenes.Setting.matchings).  Everything is compared bit for bit or byte for byte; the mirror path
(frame_window 0) to 1e-6, as the existing sequence tests compare it."""
import os

import numpy as np
import pytest
import torch

import matching_scenes as scenes
import oracle
from matching_scenes import CX, CY, FX, FY, N_SEQ, Setting, descriptor_scene, read_results, record, rgbd_kwargs, sos_kwargs
from refmatch import IDX, NONE, POPCOUNT, Matching, capped
from vo_single_camera_sos_amd import synthetic
from vo_single_camera_sos_amd.frontend import DeviceImageModel, ImageFrontEnd
from vo_single_camera_sos_amd.omnistereo.camera_models import FeatureMatcher
from vo_single_camera_sos_amd.pipeline import (FramePairBatch, FramePairPipeline, RGBDCamConfig, RGBDPairBatch, RGBDPairPipeline,
                                               RigConfig)

pytestmark = pytest.mark.gpu


class _Stage(scenes.StageProblems):
    """sosvo_match_hamming_gated on the problems, the last P - n_forward of them reversed, against the definition."""

    def __init__(self, *args, n_forward=None):
        super().__init__(*args)
        self.n_forward = self.P if n_forward is None else n_forward

    def run(self, min_dv, max_du, cap):
        keys = self.ctx.match_hamming_gated(self.d_qd, self.d_td, self.d_qp, self.d_tp, self.d_nq, self.d_nt, min_dv=min_dv,
                                            max_du=max_du, max_distance=cap, n_forward=self.n_forward, **self.sl)
        self.ctx.synchronize()
        return keys.cpu().numpy()[:, :, 0]

    def expect(self, p, min_dv, max_du, cap):
        """key(i) = min over admissible j of (hamming << 20 | j); NONE without an admissible train or beyond the cap."""
        return capped(self.smallest(p, (min_dv, max_du), p >= self.n_forward)[0], cap)

    def check(self, min_dv, max_du, cap):
        got = self.run(min_dv, max_du, cap)
        for p in range(self.P):
            want = self.expect(p, min_dv, max_du, cap)
            assert np.array_equal(got[p, : len(want)], want), (p, min_dv, max_du, cap)     # (padding rows are unspecified)
        return got


GATES = [(1.0, 2.5), (-1.0, 2.5), (1.0, 0.0), (-1.0, -1.0)]      # both sides, du alone, dv alone, neither
TRAINS = (1, 31, 32, 33, 127, 128, 129, 257)                     # 32-row blocks, 128-train tiles, a range split over tiles
QUERIES = (1, 32, 33, 128, 129)


# ---- 1. the stage -------------------------------------------------------------------------------------------------------
def test_stage_equals_the_definition_at_the_tile_edges(ctx):
    """Every (query count, train count) pair as one problem of one launch (stride 320: the train range is split over three
    workgroups), all four gate forms, caps none / 256 / 64 / 0."""
    rng = np.random.default_rng(2025)
    shapes = [(a, b) for a in QUERIES for b in TRAINS]
    S = 320
    nq, nt = np.array([s[0] for s in shapes]), np.array([s[1] for s in shapes])
    qd, qp = descriptor_scene(rng, len(shapes), S, nq)
    td, tp = descriptor_scene(rng, len(shapes), S, nt)
    td[:, ::2] = qd[:, ::2]                                       # (true partners exist: same descriptor, nearby position)
    tp[:, ::2] = qp[:, ::2] + rng.uniform(-2.0, 4.0, qp[:, ::2].shape).astype(np.float32)
    st = _Stage(ctx, qd, td, qp, tp, nq, nt)
    for (min_dv, max_du) in GATES:
        for cap in (None, 256, 64, 0):
            got = st.check(min_dv, max_du, cap)
            real = np.concatenate([got[p, : nq[p]] for p in range(st.P)])
            if cap == 0:
                assert ((real == NONE) | ((real >> 20) == 0)).all()
            elif cap == 64:
                assert (real != NONE).any() and (real == NONE).any()
    # the gate decided something: with both sides on some queries have no admissible train, with none every query has one
    both = np.concatenate([st.expect(p, 1.0, 2.5, None) for p in range(st.P)])
    none = np.concatenate([st.expect(p, -1.0, -1.0, None) for p in range(st.P)])
    assert (both == NONE).any() and (both != NONE).any() and (none != NONE).all() and (both != none).sum() > 100


def test_stage_without_gate_and_cap_equals_the_plain_matcher(ctx):
    """The two entry kernels are one search.  Second case: q_stride 1024 (two query tiles per wave, nq = 960: a dead second
    tile) against t_stride 320 as ONE problem (the train range is split over three workgroups)."""
    for seed, q_stride, nq, nt in ((3, 320, [129, 33, 300], [257, 128, 300]), (37, 1024, [960], [300])):
        rng = np.random.default_rng(seed)
        nq, nt = np.array(nq), np.array(nt)
        qd, qp = descriptor_scene(rng, len(nq), q_stride, nq)
        td, tp = descriptor_scene(rng, len(nt), 320, nt)
        st = _Stage(ctx, qd, td, qp, tp, nq, nt)
        plain = ctx.match_hamming(st.d_qd, st.d_td, st.d_nq, st.d_nt, k=1)
        ctx.synchronize()
        plain = plain.cpu().numpy()[:, :, 0]
        for cap in (None, 256):
            got = st.check(-1.0, 0.0, cap)                        # (against the oracle's keys)
            for p in range(len(nq)):
                assert np.array_equal(got[p, : nq[p]], plain[p, : nq[p]])


def test_stage_constructed_cases(ctx):
    """One problem, 8 queries against 140 trains (two tiles), gate du <= 2.5 and dv >= 1:
    query 0: no admissible train -> NONE;  query 1: its copies are trains 5 and 130, train 5 gated out -> 130 wins;
    query 2: copies at trains 7, 40 and 131, all admissible -> 7 (lowest index);  query 3: the whole first tile is gated
    out -> the winner lies in the second;  query 4: |du| == max_du and dv == min_dv exactly -> passes;  query 5: du passes,
    dv fails by one ulp -> its copy is rejected;  queries 6, 7: each side disabled on its own lets the other's failure pass."""
    rng = np.random.default_rng(17)
    S, nq, nt = 160, 8, 140
    qd = rng.integers(0, 256, (1, S, 32), dtype=np.uint8)
    td = rng.integers(0, 256, (1, S, 32), dtype=np.uint8)
    qp = np.zeros((1, S, 2), np.float32)
    tp = np.zeros((1, S, 2), np.float32)
    tp[0, :, 0] = 1000.0 + 10.0 * np.arange(S)                    # by default no train is near any query
    tp[0, :, 1] = 50.0
    qp[0, :nq, 0] = 100.0 * np.arange(nq)
    qp[0, :nq, 1] = 10.0
    # query 1
    td[0, 5] = td[0, 130] = qd[0, 1]
    tp[0, 5] = (100.0 + 2.75, 12.0)
    tp[0, 130] = (100.0 - 2.0, 12.0)
    # query 2
    td[0, 7] = td[0, 40] = td[0, 131] = qd[0, 2]
    tp[0, 7] = tp[0, 40] = tp[0, 131] = (200.0, 11.5)
    # query 3: admissible trains only at 128 .. 139, one of them at distance 3
    td[0, 135] = qd[0, 3]
    td[0, 135, 0] ^= 0x07
    tp[0, 132:140, 0] = 300.0 + np.linspace(-2.0, 2.0, 8)
    tp[0, 132:140, 1] = 20.0
    td[0, 20] = qd[0, 3]                                          # (the exact copy sits in the first tile, out of the band)
    tp[0, 20] = (303.0, 20.0)
    # query 4: the bounds themselves
    td[0, 60] = qd[0, 4]
    tp[0, 60] = (400.0 + 2.5, 11.0)
    # query 5: dv one float32 step below 1
    td[0, 61] = qd[0, 5]
    tp[0, 61] = (500.0, np.nextafter(np.float32(11.0), np.float32(0.0)))
    # queries 6 / 7
    td[0, 62] = qd[0, 6]
    tp[0, 62] = (600.0 + 30.0, 12.0)                              # du fails, dv passes
    td[0, 63] = qd[0, 7]
    tp[0, 63] = (700.0, 5.0)                                      # du passes, dv fails
    st = _Stage(ctx, qd, td, qp, tp, np.array([nq]), np.array([nt]))
    k = st.check(1.0, 2.5, None)[0, :nq]
    assert k[0] == NONE
    assert k[1] == 130 and k[2] == 7
    assert k[3] == ((3 << 20) | 135)
    assert k[4] == 60
    assert k[5] == NONE and k[6] == NONE and k[7] == NONE
    k = st.check(1.0, 0.0, None)[0, :nq]                          # du side off
    assert k[6] == 62 and k[1] == 5 and (k[7] >> 20) > 0
    k = st.check(-1.0, 2.5, None)[0, :nq]                         # dv side off
    assert k[7] == 63 and k[5] == 61 and k[6] == NONE
    k = st.check(1.0, 2.5, 2)[0, :nq]                             # the cap acts on the winner: query 3's distance is 3
    assert k[3] == NONE and k[1] == 130


def test_stage_slots_reversed_problems_and_the_unsplit_train_loop(ctx):
    """2100 problems over a store of 6 blocks (so many that the train range is not split: one workgroup walks all tiles),
    the second half reversed, as the role-swapped problems of a cross-checked step are."""
    rng = np.random.default_rng(23)
    S, counts = 320, np.array([257, 129, 128, 33, 300, 0])
    desc, pos = descriptor_scene(rng, 6, S, counts)
    P = 2100
    q_slot, t_slot = rng.integers(0, 6, P), rng.integers(0, 6, P)
    st = _Stage(ctx, desc, desc, pos, pos, counts, counts, q_slot, t_slot, n_forward=P // 2)
    st.check(1.0, 2.5, None)
    st.check(1.0, 2.5, 80)
    st.check(-1.0, 2.5, None)
    fwd = Matching(gated=True).keys(desc[1, :129], desc[0, :257], pos[1, :129], pos[0, :257], (1.0, 2.5))
    rev = Matching(gated=True).keys(desc[1, :129], desc[0, :257], pos[1, :129], pos[0, :257], (1.0, 2.5), reverse=True)
    assert not np.array_equal(fwd, rev)                           # (the reversed gate is another gate)


def test_stage_two_tiles_per_wave(ctx):
    """q_stride 1024: the kernel form with two query tiles per wave, a dead second tile included (nq = 1000 - 40)."""
    rng = np.random.default_rng(29)
    nq, nt = np.array([960]), np.array([300])
    qd, qp = descriptor_scene(rng, 1, 1024, nq)
    td, tp = descriptor_scene(rng, 1, 320, nt)
    td[0, :300:3] = qd[0, :300:3]
    tp[0, :300:3] = qp[0, :300:3] + np.float32(1.25)
    st = _Stage(ctx, qd, td, qp, tp, nq, nt)
    for (min_dv, max_du) in GATES:
        st.check(min_dv, max_du, None)
    st.check(1.0, 2.5, 64)
    assert (st.expect(0, 1.0, 2.5, None) != NONE).sum() > 100


def test_gate_is_evaluated_in_double(ctx):
    """u_t is the smallest float32 above u_q + 2.5: the exact difference exceeds max_du = 2.5, and for about half the draws
    its float32 rounding IS 2.5 -- a gate that subtracted in float32 would accept those.  Query i's only zero-distance train
    is train i, so accepting it shows in the key."""
    rng = np.random.default_rng(31)
    n = 256
    uq = rng.uniform(0.0, 1.0, n).astype(np.float32)
    uq = np.maximum(uq, np.float32(1e-3))
    s = uq.astype(np.float64) + 2.5                               # exact in double
    ut = s.astype(np.float32)
    ut = np.where(ut.astype(np.float64) <= s, np.nextafter(ut, np.float32(np.inf)), ut).astype(np.float32)
    exact = ut.astype(np.float64) - uq.astype(np.float64)
    assert (exact > 2.5).all() and (np.nextafter(ut, np.float32(0.0)).astype(np.float64) <= s).all()
    rounds_onto = (ut - uq) == np.float32(2.5)                    # float32 subtraction
    print("float32 difference rounds onto 2.5 in %d of %d draws" % (rounds_onto.sum(), n))
    assert rounds_onto.sum() >= 64                                # about half by construction (measured: see the print)
    qd = rng.integers(0, 256, (1, n, 32), dtype=np.uint8)
    td = qd.copy()
    qp = np.zeros((1, n, 2), np.float32)
    tp = np.zeros((1, n, 2), np.float32)
    qp[0, :, 0], tp[0, :, 0] = uq, ut
    tp[0, :, 1] = 1.0
    st = _Stage(ctx, qd, td, qp, tp, np.array([n]), np.array([n]))
    for min_dv in (1.0, -1.0):
        k = st.check(min_dv, 2.5, None)[0]
        assert ((k == NONE) | ((k & IDX) != np.arange(n))).all()  # nobody got its own train
        assert ((k[rounds_onto] == NONE) | ((k[rounds_onto] >> 20) > 0)).all()
    k = st.check(1.0, 2.5000005, None)[0]                         # (a hair wider and every query has it)
    assert np.array_equal(k, np.arange(n, dtype=np.uint32))


# ---- 2. FeatureMatcher.match_gated ----------------------------------------------------------------------------------------
def test_feature_matcher_match_gated(ctx):
    rng = np.random.default_rng(5)
    desc, pos = descriptor_scene(rng, 2, 320, np.array([257, 300]))
    q, t, qp, tp = desc[1, :300], desc[0, :257], pos[1, :300], pos[0, :257]
    fm = FeatureMatcher("ORB", "BF", 1, context=ctx)
    plain = fm.match(q, t)
    for cap in (None, 80, 0):
        got = fm.match_gated(q, t, qp, tp, 1.0, 2.5, max_distance=cap)
        wq, wt, wd = Matching(gated=True, cap=cap)(q, t, qp, tp, (1.0, 2.5))
        assert np.array_equal(got.query_idx, wq) and np.array_equal(got.train_idx, wt) and np.array_equal(got.distances, wd)
        assert [m.queryIdx for m in got] == list(wq) and [m.trainIdx for m in got] == list(wt)
    wq, wt, wd = Matching(gated=True)(q, t, qp, tp, (1.0, 2.5))
    assert 20 < len(wq) < 300
    # the plain matches that pass the gate are gated matches (the search under the gate can only add)
    ok = oracle.pixel_gates(tp[plain.train_idx].astype(np.float64), qp[plain.query_idx].astype(np.float64), 1.0, 2.5)
    kept = {(a, b) for a, b, o in zip(plain.query_idx, plain.train_idx, ok) if o}
    assert kept < set(zip(wq, wt))
    # without a gate and a cap it is match()
    got = fm.match_gated(q, t, qp, tp, -1.0, 0.0)
    assert np.array_equal(got.query_idx, plain.query_idx) and np.array_equal(got.train_idx, plain.train_idx)
    # [n, 3] homogeneous pixel rows are taken as they come from the frames; empty sides give no match
    got3 = fm.match_gated(q, t, np.hstack([qp, np.ones((300, 1), np.float32)]), np.hstack([tp, np.ones((257, 1), np.float32)]), 1.0, 2.5)
    assert np.array_equal(got3.query_idx, wq) and np.array_equal(got3.train_idx, wt)
    assert len(fm.match_gated(q, t[:0], qp, tp[:0], 1.0, 2.5)) == 0 and len(fm.match_gated(q[:0], t, qp[:0], tp, 1.0, 2.5)) == 0
    # mutual under the gate
    fmc = FeatureMatcher("ORB", "BF", 1, context=ctx, cross_check=True)
    got = fmc.match_gated(q, t, qp, tp, 1.0, 2.5, max_distance=80)
    wq, wt, wd = Matching(gated=True, cap=80, mutual=True)(q, t, qp, tp, (1.0, 2.5))
    assert 0 < len(wq) and np.array_equal(got.query_idx, wq) and np.array_equal(got.train_idx, wt) and np.array_equal(got.distances, wd)
    assert len(set(got.train_idx)) == len(got)


# ---- the settings --------------------------------------------------------------------------------------------------------
SETTINGS = [Setting("stereo", gate="stereo"), Setting("f2f", gate="f2f"), Setting("both", gate="both"),
            Setting("stereo_cap80", gate="stereo", cap=80), Setting("f2f_cap80", gate="f2f", cap=80),
            Setting("both_cap80", gate="both", cap=80), Setting("both_with_cross_check", gate="both", cc=True)]
OFF = Setting("off")
BY_NAME = {s.name: s for s in SETTINGS}
NAMES = [s.name for s in SETTINGS]


@pytest.fixture(scope="module")
def pairs(ctx):
    """2 rendered pairs (GFT 330 features): the front end on the GPU, the detection on the oracle (once, shared).  The
    trackers' solver settings (generalised P3P, 210 iterations with the adaptive stop) so that one reference serves the pair
    paths (pair i samples with seed + i) and the sequence engine (frame t with seed t - 1)."""
    return scenes.omni_pairs(ctx)


# ---- 3. the omni paths against the gated refflow ------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_pair_pipeline_stage_by_stage_equals_the_gated_refflow(ctx, pairs, name):
    s, setting = pairs, BY_NAME[name]
    frames, want = s.frames(setting), s.pair_tracks(setting)
    pipe = FramePairPipeline(ctx, RigConfig(**s.rig_kw), s.B, frame_cap=2048, seed=s.seed, front_end=s.fe, **s.solver,
                             **setting.omni_kw())
    pipe.stereo()
    pipe.track()
    rec = pipe.results().cpu().numpy()
    M, n_cand = pipe.frames["M"].cpu().numpy(), pipe.frames["n_cand"].cpu().numpy()
    assert [int(x) for x in M] == [len(fr["X"]) for fr in frames] and M.min() > 100
    assert [int(x) for x in n_cand] == [fr["n_cand"] for fr in frames]
    for f, fr in enumerate(frames):
        for key in ("m_top", "m_bot", "d_top", "d_bot", "X"):
            assert np.array_equal(pipe.frames[key][f, : M[f]].cpu().numpy(), fr[key]), (f, key)
    mask = pipe.ransac["mask"].cpu().numpy()
    cq, ct = pipe.corr["q"].cpu().numpy(), pipe.corr["t"].cpu().numpy()
    for i, w in enumerate(want):
        n = len(w["corr"]["cam"])
        assert n > 100 and np.array_equal(cq[i, :n], w["corr"]["q"]) and np.array_equal(ct[i, :n], w["corr"]["t"])
        assert np.array_equal(mask[i, :n].astype(bool), w["ransac"]["mask"])
        assert np.array_equal(rec[i].view(np.uint64), record(w).view(np.uint64)) and rec[i, 14] == 0
    off = s.frames(OFF)
    if setting.gate_stereo and not setting.cc and setting.cap is None:   # the search under the gate can only add stereo points
        assert all(len(a["X"]) >= len(b["X"]) for a, b in zip(frames, off))
        assert sum(len(a["X"]) for a in frames) > sum(len(b["X"]) for b in off)
    if not setting.changes_stereo:                            # the stereo stage is untouched by the f2f switch
        assert all(np.array_equal(a["X"], b["X"]) for a, b in zip(frames, off))


def test_pair_path_with_a_fraction_of_the_gated_matches(ctx, pairs):
    """pct_good_matches = 0.75 with both switches and cap 80: the gate and the cap leave many SOSVO_KEY_NONE keys, and
    int(0.75 * len(matches)) counts the REAL matches per bucket and per view, in the stage path and behind the one C call."""
    s, setting = pairs, BY_NAME["both_cap80"]
    rig_kw = dict(s.rig_kw, pct_good_matches=0.75)
    pipe = FramePairPipeline(ctx, RigConfig(**rig_kw), s.B, frame_cap=2048, seed=s.seed, front_end=s.fe, **s.solver,
                             **setting.omni_kw())
    pipe.stereo()
    pipe.track()
    rec = pipe.results().cpu().numpy()
    frames, want = s.frames(setting, pct=0.75), s.pair_tracks(setting, pct=0.75)
    full = s.frames(setting)
    M, n_cand = pipe.frames["M"].cpu().numpy(), pipe.frames["n_cand"].cpu().numpy()
    assert [int(x) for x in M] == [len(fr["X"]) for fr in frames]
    assert [int(x) for x in n_cand] == [fr["n_cand"] for fr in frames]
    assert all(0 < a["n_cand"] < b["n_cand"] for a, b in zip(frames, full))      # the fraction bites in every frame
    mask = pipe.ransac["mask"].cpu().numpy()
    cq, ct = pipe.corr["q"].cpu().numpy(), pipe.corr["t"].cpu().numpy()
    for i, w in enumerate(want):
        n = len(w["corr"]["cam"])
        assert n > 0 and np.array_equal(cq[i, :n], w["corr"]["q"]) and np.array_equal(ct[i, :n], w["corr"]["t"])
        assert np.array_equal(mask[i, :n].astype(bool), w["ransac"]["mask"])
        assert np.array_equal(rec[i].view(np.uint64), record(w).view(np.uint64))
    batch = FramePairBatch(ctx, s.model, RigConfig(**rig_kw), s.B, num_of_features=s.nfeat, kp_cap=s.fe.kp_cap, frame_cap=2048,
                           seed=s.seed, **s.solver, **setting.omni_kw())
    batch.load_frames(s.omni)
    got = batch.step()
    ctx.synchronize()
    assert np.array_equal(got.cpu().numpy().view(np.uint64), rec.view(np.uint64))


@pytest.mark.parametrize("name", NAMES)
def test_one_call_batches_equal_the_gated_refflow(ctx, pairs, name):
    s, setting = pairs, BY_NAME[name]
    want = np.stack([record(w) for w in s.pair_tracks(setting)])
    kw = dict(num_of_features=s.nfeat, kp_cap=s.fe.kp_cap, frame_cap=2048, seed=s.seed, **s.solver, **setting.omni_kw())
    for ns in (1, 2):
        batch = FramePairBatch(ctx, s.model, RigConfig(**s.rig_kw), s.B, n_streams=ns, **kw)
        batch.workspace.fill_(0xA5)
        batch.load_frames(s.omni)
        for _ in range(2):
            got = batch.step().clone()
            ctx.synchronize()
            assert np.array_equal(got.cpu().numpy().view(np.uint64), want.view(np.uint64)), ns
        if ns == 2:                                          # the enqueue / join form
            bufs = [torch.zeros_like(batch.out), torch.zeros_like(batch.out)]
            for k in range(4):
                batch.enqueue(bufs[k & 1])
            batch.join()
            ctx.synchronize()
            for b in bufs:
                assert np.array_equal(b.cpu().numpy().view(np.uint64), want.view(np.uint64))
    assert not np.array_equal(want[:, :12], np.stack([record(w) for w in s.pair_tracks(OFF)])[:, :12])


@pytest.mark.parametrize("name", NAMES)
def test_sequence_engine_equals_the_gated_refflow_for_windows_1_and_5(ctx, pairs, name):
    from vo_single_camera_sos_amd.pipeline import MultiSequenceEngine, SequenceEngine
    s, setting = pairs, BY_NAME[name]
    want = np.stack([record(w) for w in s.hop_tracks(setting)])
    kw = dict(num_of_features=s.nfeat, kp_cap=s.fe.kp_cap, frame_cap=2048, **s.solver, **setting.omni_kw())
    n = 2 * s.B
    for window in (1, 5):
        eng = SequenceEngine(ctx, s.model, RigConfig(**s.rig_kw), window=window, **kw)
        got = scenes.hop_records(eng, s.omni[:n], window)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), window
    assert MultiSequenceEngine(ctx, s.model, RigConfig(**s.rig_kw), lanes=2, window=2, **kw).cfg.ransac_flags == eng.cfg.ransac_flags


# ---- 4. RGB-D --------------------------------------------------------------------------------------------------------------
RGBD_SETTINGS = [Setting("f2f", gate="f2f"), Setting("f2f_cap80", gate="f2f", cap=80),
                 Setting("f2f_with_cross_check", gate="f2f", cc=True)]


@pytest.fixture(scope="module")
def rgbd(ctx):
    return scenes.rgbd_pairs(ctx)


@pytest.mark.parametrize("setting", RGBD_SETTINGS, ids=[x.name for x in RGBD_SETTINGS])
def test_rgbd_pair_paths_and_sequence_equal_the_gated_refflow(ctx, rgbd, setting):
    from vo_single_camera_sos_amd.pipeline import RGBDSequenceEngine
    s = rgbd
    want = [s.track(setting, 2 * i, 2 * i + 1, 31 + i) for i in range(s.B)]
    want_seq = np.stack([record(s.track(setting, t - 1, t, t - 1)) for t in range(1, 2 * s.B)])
    plain = [s.track(None, 2 * i, 2 * i + 1, 31 + i) for i in range(s.B)]
    pipe = RGBDPairPipeline(ctx, s.cam, s.B, seed=31, **s.kw, **setting.rgbd_kw())
    pipe.load_frames(s.bgr, s.depth)
    pipe.step()
    rec, mask = pipe.results().cpu().numpy(), pipe.ransac["mask"].cpu().numpy()
    cq, ct = pipe.corr["q"].cpu().numpy(), pipe.corr["t"].cpu().numpy()
    for i, w in enumerate(want):
        n = len(w["corr"]["q"])
        assert n > 100 and np.array_equal(cq[i, :n], w["corr"]["q"]) and np.array_equal(ct[i, :n], w["corr"]["t"])
        assert np.array_equal(mask[i, :n].astype(bool), w["ransac"]["mask"])
        assert np.array_equal(rec[i].view(np.uint64), record(w).view(np.uint64)) and rec[i, 14] == 0
        if not setting.cc and setting.cap is None:           # the plain correspondences are a subset of the gated ones
            assert set(zip(plain[i]["corr"]["q"], plain[i]["corr"]["t"])) < set(zip(w["corr"]["q"], w["corr"]["t"]))
    one = RGBDPairBatch(ctx, s.cam, s.B, seed=31, **s.kw, **setting.rgbd_kw())
    one.load_frames(s.bgr, s.depth)
    got = one.step()
    ctx.synchronize()
    assert np.array_equal(got.cpu().numpy().view(np.uint64), rec.view(np.uint64))
    for window in (1, 5):
        eng = RGBDSequenceEngine(ctx, s.cam, window=window, **s.kw, **setting.rgbd_kw())
        got = scenes.hop_records(eng, list(zip(s.bgr, s.depth)), window)
        assert np.array_equal(got.view(np.uint64), want_seq.view(np.uint64)), window


def test_rgbd_refuses_gated_stereo(ctx):
    from vo_single_camera_sos_amd import _lib
    from vo_single_camera_sos_amd.device import SosvoError
    cam = RGBDCamConfig(fx=FX, fy=FY, center_x=CX, center_y=CY, depth_is_Z=True, min_range=0.8, max_range=7.0)
    one = RGBDPairBatch(ctx, cam, 1, num_of_features=100)
    one.cfg.flags |= _lib.FLAG_GATED_STEREO
    with pytest.raises(SosvoError, match="SOSVO_FLAG_GATED_STEREO"):
        one.step()


# ---- 5. run_VO: the sequence engines, the mirror path, run_VO_many -------------------------------------------------------
@pytest.fixture(scope="module")
def sos_sequences(tmp_path_factory):
    return scenes.write_sos_sequences(tmp_path_factory.mktemp("gated_sos"))


@pytest.mark.parametrize("name", NAMES)
def test_run_vo_windows_and_mirror_path(ctx, sos_sequences, tmp_path, name):
    """The pose file is byte-identical for frame windows 5 and 1, and the per-frame mirror path (frame_window 0: the
    FeatureMatcher objects of the camera model, match_features_panoramic_top_bottom / match_features_frame_to_frame) gives
    the same poses to rounding and the same keyframes."""
    from vo_single_camera_sos_amd.omnistereo.gum import load_gums_json
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import run_VO
    seq, kw = sos_sequences[0], BY_NAME[name].run_vo_kw()
    model = load_gums_json(os.path.join(seq, "gums-calibrated.json"))
    files, outs = scenes.run_vo_windows(model, seq, N_SEQ, tmp_path, (5, 1, 0), **kw)
    assert files[5] == files[1] and "sequence_mode" in outs[5] and "sequence_mode" not in outs[0]
    for (i, Ta), (j, Tb) in zip(outs[0]["poses"], outs[5]["poses"]):
        assert i == j and np.allclose(Ta, Tb, rtol=1e-6, atol=1e-9), (i, np.abs(Ta - Tb).max())
    assert outs[0]["keyframe_ids"] == outs[5]["keyframe_ids"]
    res = str(tmp_path / "off")
    off = run_VO(None, model, frame_window=5, gated_matching=False, **sos_kwargs(seq, N_SEQ, res))
    assert off["tracked"] == N_SEQ - 1 and read_results(res)[0] != files[5][0]
    res = str(tmp_path / "none")                             # None is the tracker's own setting: off
    run_VO(None, model, frame_window=5, gated_max_distance=80, **sos_kwargs(seq, N_SEQ, res))
    assert read_results(res) == read_results(str(tmp_path / "off"))


@pytest.mark.parametrize("name", NAMES)
def test_run_vo_many_equals_the_solo_runs(ctx, sos_sequences, tmp_path, name):
    gums = os.path.join(sos_sequences[0], "gums-calibrated.json")
    want, outs = scenes.run_vo_many_against_solo(gums, sos_sequences, N_SEQ, tmp_path, **BY_NAME[name].run_vo_kw())
    assert all(o["sequence_mode"]["lanes"] == 2 for o in outs)
    assert want[0] != want[1]


def test_rgbd_run_vo(ctx, tmp_path):
    from vo_single_camera_sos_amd.omnistereo.camera_models import RGBDCamModel
    from vo_single_camera_sos_amd.omnistereo.pose_est_tools import run_VO
    from vo_single_camera_sos_amd.omnistereo.transformations import rotation_matrix
    seq = str(tmp_path / "seq_rgbd")
    synthetic.write_rgbd_sequence(seq, n_frames=N_SEQ, seed=41, max_t=40.0, max_deg=2.0, depth_is_Z=False)
    model = RGBDCamModel(fx=FX, fy=FY, center_x=CX, center_y=CY, scaling_factor=1. / 1000.0, do_undistortion=False,
                         depth_is_Z=False, focal_length_m=1. / 1000.0)
    model.T_Cest_wrt_Rgt = rotation_matrix(-np.pi / 2.0, [1, 0, 0])
    files, outs = {}, {}
    for w in (5, 1, 0):
        res = str(tmp_path / ("w%d" % w))
        outs[w] = run_VO(None, model, frame_window=w, gated_matching=True, gated_max_distance=80, **rgbd_kwargs(seq, N_SEQ, res))
        files[w] = read_results(res)
        assert outs[w]["tracked"] == N_SEQ - 1
    assert files[5] == files[1]
    for (i, Ta), (_, Tb) in zip(outs[5]["poses"], outs[0]["poses"]):
        assert np.allclose(Ta, Tb, rtol=1e-9, atol=1e-12), (i, np.abs(Ta - Tb).max())
    res = str(tmp_path / "off")
    run_VO(None, model, frame_window=5, **rgbd_kwargs(seq, N_SEQ, res))
    assert read_results(res)[0] != files[5][0]
    with pytest.raises(ValueError, match="no static-stereo matcher"):
        run_VO(None, model, frame_window=5, gated_matching="stereo", **rgbd_kwargs(seq, N_SEQ, str(tmp_path / "bad")))


# ---- 6. the relations of the definition ---------------------------------------------------------------------------------------
def _hamming_rows(a, b):
    return POPCOUNT[a ^ b].sum(-1)


def test_plain_matches_are_a_subset_of_the_gated_ones_on_the_six_rendered_pairs(ctx):
    """The six rendered pairs of test_gpu_cross_check.py (seed 4100, GFT 1000 features, kp_cap 512, frame_cap 2048: no
    capacity is reached).  Without a cap the plain stereo survivors of every frame are among the gated ones, and the plain
    frame-to-frame (query, train) pairs of every pair and view among the gated ones; with cap 80 the same holds for the plain
    matches whose distance is within the cap."""
    B = 6
    gs, rig_kw = scenes.rig()
    omni, _ = synthetic.make_frame_pairs(gs, B, seed=4100)
    model = DeviceImageModel(ctx, gs, (480, 640))
    fe = ImageFrontEnd(ctx, model, 2 * B, detection_method="GFT", num_of_features=1000, kp_cap=512)
    fe.load_frames(omni)
    fe.run()

    def run(**kw):
        pipe = FramePairPipeline(ctx, RigConfig(**rig_kw), B, frame_cap=2048, max_iter=200, seed=11, front_end=fe, **kw)
        pipe.stereo()
        pipe.track()
        ctx.synchronize()
        fr = {k: v.cpu().numpy() for k, v in pipe.frames.items()}
        co = {k: v.cpu().numpy() for k, v in pipe.corr.items()}
        assert fr["M"].max() < 2048 and co["n"].max() < 4096    # neither frame_cap nor the correspondence capacity is reached
        stereo = []
        for f in range(2 * B):
            m = int(fr["M"][f])
            rows = np.hstack([fr["m_top"][f, :m], fr["m_bot"][f, :m]])
            stereo.append(dict(zip(map(bytes, rows), _hamming_rows(fr["d_top"][f, :m], fr["d_bot"][f, :m]))))
        f2f = []
        for i in range(B):
            n, nt = int(co["n"][i]), int(co["n_top"][i])
            views = []
            for view, (lo, hi) in enumerate(((0, nt), (nt, n))):
                d = fr["d_top" if view == 0 else "d_bot"]
                q, t = co["q"][i, lo:hi], co["t"][i, lo:hi]
                views.append(dict(zip(zip(q.tolist(), t.tolist()), _hamming_rows(d[2 * i + 1][q], d[2 * i][t]))))
            f2f.append(views)
        return stereo, f2f
    plain_s, plain_f = run()
    for cap in (None, 80):
        gated_s, _ = run(gated_stereo=True, gated_max_distance=cap)
        _, gated_f = run(gated_f2f=True, gated_max_distance=cap)      # (on the plain frames: the same train and query sets)
        within = (lambda d: True) if cap is None else (lambda d: d <= cap)
        for f in range(2 * B):
            assert {k for k, d in plain_s[f].items() if within(d)} <= set(gated_s[f]), (cap, f)
            assert cap is None or max(gated_s[f].values()) <= cap
        for i in range(B):
            for view in range(2):
                assert {k for k, d in plain_f[i][view].items() if within(d)} <= set(gated_f[i][view]), (cap, i, view)
        print("cap %s: stereo points per frame plain %s gated %s; correspondences per pair plain %s gated %s" % (
            cap, [len(x) for x in plain_s], [len(x) for x in gated_s], [len(a) + len(b) for a, b in plain_f],
            [len(a) + len(b) for a, b in gated_f]))
    assert min(len(x) for x in plain_s) > 300
