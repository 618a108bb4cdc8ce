"""Host logic of the multi-sequence engines (pipeline._MultiSequenceBase and its lanes) on the CPU, with the device calls
replaced by a recorder as in test_sequence_bookkeeping.py: where the lanes' slots lie in the shared store, what the slot
tables of the front end hold, that a promoted frame's copy is issued before its half is refilled, that the requests of S
lanes become ONE call each with the concatenated pairs and the per-pair seeds of the serial loops, that a lane which
finishes early does not stall a round, and how run_VO_many shards a list of sequences."""
import contextlib
import threading

import pytest
import torch

from vo_single_camera_sos_amd import parallel
from vo_single_camera_sos_amd.omnistereo import pose_est_tools
from vo_single_camera_sos_amd.pipeline import _MultiSequenceBase


class _Stream(object):
    def wait_event(self, ev):
        pass


class _Ctx(object):
    stream = _Stream()
    device = "cpu"

    def synchronize(self):
        pass


class _Ev(object):
    def record(self, stream=None):
        pass

    def elapsed_time(self, other):
        return 0.0


class Recorder(_MultiSequenceBase):
    """Frames are (lane, t) tuples coded as 1000 * lane + t; a slot of the store holds the frame written there; a tracking
    record is (ref frame, cur frame, seed)."""
    cfg = None

    def __init__(self, lanes, window):
        self.ctx = _Ctx()
        self.log, self.store = [], {}
        self._init_lanes(lanes, window)
        self.staged = {(s, b): [] for s in range(self.S) for b in (0, 1)}
        self.spec = torch.zeros((self.window, 16), dtype=torch.float64)
        self.spec2 = torch.zeros((self.window, 16), dtype=torch.float64)
        self.serial = torch.zeros((self.S, 16), dtype=torch.float64)
        self._make_lanes()

    def _stream_scope(self):
        return contextlib.nullcontext()

    @staticmethod
    def _timing_events():
        return _Ev(), _Ev()

    def _stage_lane(self, s, images, buf):
        self.staged[(s, buf)] = list(images)

    def _front_end_round(self, requests, slot_of_frame):
        frames = [f for s, buf, n in requests for f in self.staged[(s, buf)][:n]]
        assert len(frames) == len(slot_of_frame)
        self.log.append(("front_end", tuple(requests), tuple(slot_of_frame)))
        for f, slot in zip(frames, slot_of_frame):
            self.store[slot] = f

    def _track_seeds(self, ref_slots, cur_slots, seeds, out):
        assert len(ref_slots) == len(cur_slots) == len(seeds) <= out.shape[0]
        for k, (r, c, sd) in enumerate(zip(ref_slots, cur_slots, seeds)):
            out[k, 0], out[k, 1], out[k, 2] = self.store[r], self.store[c], sd
        self.log.append(("track", tuple(ref_slots), tuple(cur_slots), tuple(seeds)))

    def _counts_all(self):
        return [100 + self.store.get(slot, -100) for slot in range(self.slots)]

    def _copy_slots(self, src, dst):
        self.log.append(("copy", tuple(src), tuple(dst)))
        for a, b in zip(src, dst):
            self.store[b] = self.store[a]


def _frame(lane, t):
    return 1000 * lane + t


def _windows(n, w):
    return [list(range(k, min(n, k + w))) for k in range(0, n, w)]


@pytest.mark.parametrize("lanes,window", [(1, 4), (3, 1), (3, 4), (5, 3)])
def test_lane_slots_are_disjoint_and_inside_the_store(lanes, window):
    eng = Recorder(lanes, window)
    assert eng.slots == lanes * (2 * window + 1) and eng.window == lanes * window
    seen = set()
    for s in range(lanes):
        lane = eng.lane(s)
        own = set(range(lane._slot0, lane._slot0 + 2 * window + 1))
        assert lane.key_slot == lane._slot0 + 2 * window and lane.W == window
        assert not (own & seen) and max(own) < eng.slots and min(own) >= 0
        seen |= own
    assert seen == set(range(eng.slots))


def _lockstep(eng, lengths, window, on_frame=None):
    """Drives the lanes from ONE thread the way S run_VO loops would in lockstep: every live lane files its window, then
    every one collects (the first collect serves the round).  -> per lane, the list of window infos in order."""
    S = len(lengths)
    chunks = [_windows(n, window) for n in lengths]
    infos = [[] for _ in range(S)]
    for k in range(max(len(c) for c in chunks)):
        live = [s for s in range(S) if k < len(chunks[s])]
        for s in live:
            eng.lane(s).stage_host([_frame(s, t) for t in chunks[s][k]], k % 2)
            eng.lane(s).enqueue_staged(k % 2, len(chunks[s][k]))
        for s in live:
            got = eng.lane(s).collect()
            infos[s] += got
            if on_frame is not None:
                for info, t in zip(got, chunks[s][k]):
                    on_frame(s, t, info)
    return infos


@pytest.mark.parametrize("window", [1, 3, 4])
def test_requests_of_all_lanes_become_one_call_with_the_serial_loops_triples(window):
    lengths = [11, 7, 9]
    eng = Recorder(3, window)
    infos = _lockstep(eng, lengths, window)
    for s, n in enumerate(lengths):
        assert len(infos[s]) == n
        for t, info in enumerate(infos[s]):
            assert info["count"] == 100 + _frame(s, t) and info["seed"] == max(t - 1, 0)
            assert eng.lane(s)._slot0 <= info["slot"] < eng.lane(s)._slot0 + 2 * window
            if t == 0:
                assert info["spec"] is None
            else:       # frame t against its predecessor with seed t - 1
                assert tuple(info["spec"][:3]) == (_frame(s, t - 1), _frame(s, t), t - 1)
            if info["spec2"] is not None:
                assert tuple(info["spec2"][:3]) == (_frame(s, t - 2), _frame(s, t), t - 1)
    fe = [e for e in eng.log if e[0] == "front_end"]
    rounds = max(len(_windows(n, window)) for n in lengths)
    assert len(fe) == rounds == eng.counters["front_end_launches"] == eng.counters["rounds"]    # one per round, not per lane
    for e in fe:
        assert len(set(e[2])) == len(e[2]) and all(0 <= v < eng.slots for v in e[2])            # no slot twice
        assert sum(n for _, _, n in e[1]) == len(e[2])
    # the first round holds a window of every lane; its first-guess call holds the pairs of all of them, concatenated
    assert [s for s, _, _ in fe[0][1]] == [0, 1, 2]
    tr = [e for e in eng.log if e[0] == "track"]
    assert eng.counters["speculative_track_launches"] == len(tr) <= 2 * rounds
    if window > 1:
        lanes_in_first = {eng.store[c] // 1000 for c in tr[0][2]}
        assert lanes_in_first == {0, 1, 2}


def test_per_pair_seeds_follow_each_lanes_own_frame_counter():
    """Lanes at different positions of their sequences share a call: the seeds are t_s - 1 per lane, not seed + i."""
    eng = Recorder(2, 2)
    # lane 0 runs two windows alone, then both lanes file a window into the same round
    lane0, lane1 = eng.lane(0), eng.lane(1)
    for k in range(2):
        lane0.stage_host([_frame(0, 2 * k), _frame(0, 2 * k + 1)], k % 2)
        lane0.push_staged(k % 2, 2)
    del eng.log[:]
    lane0.stage_host([_frame(0, 4), _frame(0, 5)], 0)
    lane1.stage_host([_frame(1, 0), _frame(1, 1)], 0)
    lane0.enqueue_staged(0, 2)
    lane1.enqueue_staged(0, 2)
    lane0.collect()
    lane1.collect()
    tr = [e for e in eng.log if e[0] == "track"]
    assert len(tr) == 2 and len([e for e in eng.log if e[0] == "front_end"]) == 1
    first = {(eng.store[r], eng.store[c]): sd for r, c, sd in zip(*tr[0][1:])}
    assert first == {(_frame(0, 3), _frame(0, 4)): 3, (_frame(0, 4), _frame(0, 5)): 4, (_frame(1, 0), _frame(1, 1)): 0}
    second = {(eng.store[r], eng.store[c]): sd for r, c, sd in zip(*tr[1][1:])}
    assert second == {(_frame(0, 2), _frame(0, 4)): 3, (_frame(0, 3), _frame(0, 5)): 4}


def test_serial_requests_pending_together_are_one_call_and_promotions_one_copy():
    eng = Recorder(3, 2)
    _lockstep(eng, [2, 2, 2], 2)
    del eng.log[:]
    # every lane promotes its frame 0 and asks for frame 1 against its keyframe slot with its own seed
    for s in range(3):
        lane = eng.lane(s)
        lane.promote(lane._slot0 + 0)
        with eng._cv:
            lane._flush_promotion()
            lane._track_req = (lane.key_slot, lane._slot0 + 1, 40 + s)
    rec = eng.lane(0).track(eng.lane(0).key_slot, eng.lane(0)._slot0 + 1, 40)     # (re-files lane 0's; serves all three)
    assert tuple(rec[:3]) == (_frame(0, 0), _frame(0, 1), 40)
    assert [e[0] for e in eng.log] == ["copy", "track"]                           # copies first, then ONE tracking call
    assert eng.log[0][1] == tuple(eng.lane(s)._slot0 for s in range(3))
    assert eng.log[0][2] == tuple(eng.lane(s).key_slot for s in range(3))
    assert eng.log[1][3] == (40, 41, 42)
    for s in (1, 2):
        assert tuple(eng.lane(s)._track_res[:3]) == (_frame(s, 0), _frame(s, 1), 40 + s)
    assert eng.counters["serial_track_launches"] == 1 and eng.counters["max_serial_pairs"] == 3
    assert eng.counters["copy_launches"] == 1


@pytest.mark.parametrize("window", [1, 2, 3])
def test_a_promoted_frames_copy_is_issued_before_its_half_is_refilled(window):
    """Per lane: the last frame of window 0 is promoted and nothing reads the keyframe slot for three more windows, the
    second of which refills the promoted frame's half.  The copy to the lane's keyframe slot is in the log before the
    front-end call that overwrites the frame's slot, and a serial call against the keyframe slot then sees that frame."""
    eng = Recorder(2, window)
    promoted = {}

    def on_frame(s, t, info):
        if t == window - 1:
            eng.lane(s).promote(info["slot"])
            promoted[s] = info["slot"]
    infos = _lockstep(eng, [4 * window, 4 * window], window, on_frame)
    for s in range(2):
        src = promoted[s]
        copy_at = [i for i, e in enumerate(eng.log) if e[0] == "copy" and src in e[1]]
        writes = [i for i, e in enumerate(eng.log) if e[0] == "front_end" and src in e[2]]
        assert len(copy_at) == 1 and len(writes) == 2 and writes[0] < copy_at[0] < writes[1]
        e = eng.log[copy_at[0]]
        assert e[2][e[1].index(src)] == eng.lane(s).key_slot
        rec = eng.lane(s).track(eng.lane(s).key_slot, infos[s][-1]["slot"], 4 * window - 2)
        assert tuple(rec[:3]) == (_frame(s, window - 1), _frame(s, 4 * window - 1), 4 * window - 2)
    # both lanes' copies were due in the same round: one launch
    assert eng.counters["copy_launches"] == 1


def test_a_lane_that_finishes_early_does_not_stall_a_round():
    """Three lanes on three threads; lane 1 ends after its first window.  The others' rounds go on without it."""
    eng = Recorder(3, 2)
    lengths, done, errors = [8, 2, 6], {}, []

    def work(s):
        try:
            lane = eng.begin(s)
            out = []
            for k, chunk in enumerate(_windows(lengths[s], 2)):
                lane.stage_host([_frame(s, t) for t in chunk], k % 2)
                out += lane.push_staged(k % 2, len(chunk))
                if k > 0:   # a serial call per window, against the keyframe slot (frame 0 promoted in window 0)
                    rec = lane.track(lane.key_slot, out[-1]["slot"], len(out) - 2)
                    assert tuple(rec[:3]) == (_frame(s, 0), _frame(s, len(out) - 1), len(out) - 2)
                else:
                    lane.promote(out[0]["slot"])
            done[s] = out
        except BaseException as e:  # noqa: B902
            errors.append(e)
        finally:
            eng.end(s)
    threads = [threading.Thread(target=work, args=(s,)) for s in range(3)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=60)
    assert not any(th.is_alive() for th in threads), "a round waited for a lane that had finished"
    assert not errors, errors
    for s, n in enumerate(lengths):
        assert [i["count"] for i in done[s]] == [100 + _frame(s, t) for t in range(n)]
    assert eng.counters["front_end_launches"] <= sum(len(_windows(n, 2)) for n in lengths)
    assert not eng._live and not eng._parked


@pytest.mark.parametrize("window", [1, 3])
def test_lanes_on_threads_advance_in_lockstep(window):
    """All lanes live before the first one parks: every serve then holds one request of every live lane -- one front-end
    call per round and one serial call per step, however the threads are scheduled (a lane that has been served and files
    its next request before the others have woken up does not take them for parked)."""
    lengths = [7, 4, 9]
    for _ in range(20):
        eng = Recorder(3, window)
        errors = []

        def work(s):
            try:
                lane, t = eng.lane(s), 0
                for k, chunk in enumerate(_windows(lengths[s], window)):
                    lane.stage_host([_frame(s, u) for u in chunk], 0)
                    for info in lane.push_staged(0, len(chunk)):
                        if t == 0:
                            lane.promote(info["slot"])
                        else:
                            rec = lane.track(lane.key_slot, info["slot"], info["seed"])
                            assert tuple(rec[:3]) == (_frame(s, 0), _frame(s, t), t - 1)
                        t += 1
            except BaseException as e:  # noqa: B902
                errors.append(e)
            finally:
                eng.end(s)
        for s in range(3):
            eng.begin(s)
        threads = [threading.Thread(target=work, args=(s,)) for s in range(3)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(timeout=60)
        assert not any(th.is_alive() for th in threads) and not errors, errors
        c = eng.counters
        assert c["front_end_launches"] == c["rounds"] == max(len(_windows(n, window)) for n in lengths), c
        assert c["serial_track_launches"] == max(lengths) - 1 and c["max_serial_pairs"] == 3 and c["copy_launches"] == 1, c


def test_a_failing_device_call_wakes_every_lane():
    eng = Recorder(2, 2)

    def boom(*a):
        raise OSError("device call failed")
    eng._front_end_round = boom
    errors = []

    def work(s):
        try:
            lane = eng.begin(s)
            lane.stage_host([_frame(s, 0)], 0)
            lane.push_staged(0, 1)
        except BaseException as e:  # noqa: B902
            errors.append(e)
        finally:
            try:
                eng.end(s)
            except BaseException:  # noqa: B902
                pass
    threads = [threading.Thread(target=work, args=(s,)) for s in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=60)
    assert not any(th.is_alive() for th in threads)
    assert len(errors) == 2 and eng._error is not None


def test_shards_take_shard_ranges_blocks_and_partition_the_list(monkeypatch):
    calls = []

    def fake_run_VO(visualizer, camera_model, **kw):
        calls.append(kw["results_path"])
        return dict(poses=[], keyframe_ids=[], tracked=0, message=kw["results_path"])
    monkeypatch.setattr(pose_est_tools, "run_VO", fake_run_VO)
    seqs = [dict(img_filename_template="t%d" % i, results_path="r%d" % i) for i in range(7)]
    for world in (1, 2, 3, 4, 8):
        taken = []
        for rank in range(world):
            del calls[:]
            out = pose_est_tools.run_VO_many(object(), seqs, frame_window=4, shard=(rank, world), lanes=2)
            lo, hi = parallel.shard_range(len(seqs), rank, world)
            assert [o["message"] for o in out] == ["r%d" % i for i in range(lo, hi)]
            assert sorted(calls) == sorted("r%d" % i for i in range(lo, hi))
            taken += [o["message"] for o in out]
        assert taken == ["r%d" % i for i in range(7)]
    assert pose_est_tools.run_VO_many(object(), seqs[:2], frame_window=4, shard=(3, 4)) == []


def test_lane_limit_and_bad_arguments():
    assert pose_est_tools._lane_limit(3, None, 32) == 3
    assert pose_est_tools._lane_limit(3, 2, 32) == 2
    assert pose_est_tools._lane_limit(1000, None, 32) == 8192 // 32
    assert pose_est_tools._lane_limit(100000, None, 1) == min(8192, 65535 // 3)
    with pytest.raises(ValueError):
        pose_est_tools.run_VO_many(object(), [dict(img_filename_template="a", results_path="r")], frame_window=0)
    with pytest.raises(ValueError):
        pose_est_tools.run_VO_many(object(), [dict(results_path="r")], frame_window=4)
    with pytest.raises(ValueError):     # an omnistereo model with a depth template: SOS and RGB-D do not mix
        pose_est_tools.run_VO_many(object(), [dict(img_filename_template="a", depth_filename_template="d", results_path="r")],
                                   frame_window=4)
