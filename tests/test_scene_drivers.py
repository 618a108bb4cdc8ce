"""The drivers of tests/matching_scenes.py on the CPU: drive_lanes and assert_same_drive on the recorder engine of
test_multi_sequence_bookkeeping.py (frames are codes, a tracking record is (ref frame, cur frame, seed)), hop_records on a
stub engine."""
import numpy as np
import pytest

import matching_scenes as scenes
from test_multi_sequence_bookkeeping import Recorder, _frame


def _sequences(lengths):
    return [[_frame(k, t) for t in range(n)] for k, n in enumerate(lengths)]


def test_drive_lanes_returns_each_lanes_drive():
    seqs = _sequences([4, 3])
    eng = Recorder(2, 2)
    got = scenes.drive_lanes(eng, seqs, 2)
    assert not eng._live
    for k, frames in enumerate(seqs):
        assert len(got[k]) == len(frames)
        for t, (count, seed, spec, _, rec) in enumerate(got[k]):
            assert count == 100 + frames[t] and seed == max(t - 1, 0)
            if t == 0:                                           # promoted: nothing to track against
                assert spec is None and rec is None
                continue
            assert tuple(spec[:3]) == (frames[t - 1], frames[t], t - 1)
            assert tuple(rec[:3]) == (frames[0], frames[t], t - 1)
        scenes.assert_same_drive(got[k], scenes.drive(Recorder(1, 2).lane(0), frames, 2))


def test_drive_lanes_raises_a_lanes_exception_after_every_lane_has_ended():
    seqs = _sequences([4, 3])
    eng = Recorder(2, 2)
    ended, end, push = [], eng.end, eng.lane(1).push_window

    def failing_push(images):
        if images[0] == seqs[1][2]:                              # lane 1's second window
            raise OSError("lane 1 cannot read its frame")
        return push(images)

    def recording_end(k):
        ended.append(k)
        end(k)
    eng.lane(1).push_window, eng.end = failing_push, recording_end
    with pytest.raises(OSError, match="lane 1 cannot read"):
        scenes.drive_lanes(eng, seqs, 2)
    assert sorted(ended) == [0, 1] and not eng._live
    assert set(seqs[0]) <= set(eng.store.values())               # lane 0 was not left waiting: its four frames went through


class _Hops(object):
    """push_window -> infos whose spec is (previous frame, frame), None for the sequence's first frame."""

    def __init__(self):
        self.windows, self.last = [], None

    def push_window(self, frames):
        self.windows.append(len(frames))
        infos = []
        for f in frames:
            infos.append(dict(spec=None if self.last is None else np.array([self.last, f], dtype=np.float64)))
            self.last = f
        return infos


def test_hop_records_are_in_frame_order_over_a_ragged_last_window():
    eng = _Hops()
    got = scenes.hop_records(eng, np.arange(10, 15), 2)
    assert eng.windows == [2, 2, 1]
    assert np.array_equal(got, [[10, 11], [11, 12], [12, 13], [13, 14]])
    got = scenes.hop_records(_Hops(), [(b, -b) for b in range(3)], 5)         # a list of tuples, as the RGB-D engines take
    assert got.shape == (2, 2, 2) and np.array_equal(got[1], [[1, -1], [2, -2]])


def test_assert_same_drive():
    def a_drive():
        rec = lambda *v: np.array(v, dtype=np.float64)  # noqa: E731
        return [(100, 0, None, None, None), (101, 0, rec(0, 1, 0), None, rec(0, 1, 0)),
                (102, 1, rec(1, 2, 1), rec(0, 2, 1), rec(0, 2, 1))]
    scenes.assert_same_drive(a_drive(), a_drive())
    other = a_drive()
    other[2][3][1] = np.nextafter(other[2][3][1], 3.0)           # one element of one record, by one ulp
    with pytest.raises(AssertionError):
        scenes.assert_same_drive(a_drive(), other)
    other = a_drive()
    other[1] = other[1][:3] + (other[1][4], other[1][4])         # a record where the other drive has None
    with pytest.raises(AssertionError):
        scenes.assert_same_drive(a_drive(), other)
    other = a_drive()
    other[2] = (102, 2) + other[2][2:]                           # another seed
    with pytest.raises(AssertionError):
        scenes.assert_same_drive(a_drive(), other)
    with pytest.raises(AssertionError):                          # a drive that stopped a frame early
        scenes.assert_same_drive(a_drive(), a_drive()[:2])
