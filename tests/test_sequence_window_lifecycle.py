"""Host logic of run_VO's sequence mode on the CPU: the window generator (pose_est_tools.sequence_windows) and its staging
thread, with the engine replaced by a fake that logs every call with the run it was made in (reset() starts a new run, as
sequence_engine_for does when it hands a cached engine to the next run).  What must hold however a run ends -- closed by
the consumer, the consumer raising, the source raising, the source blocking -- is that once the generator has been closed
no call from that run reaches the engine: the next run with the same camera model gets the same engine, and a stale
upload would put the previous run's frames into its buffers.  Each interleaving is forced with events, not with timing:
the engine's stage_host can be held on a gate that the generator's stop event opens, and the source can block on an event
the test sets."""
import contextlib
import threading

import pytest

from vo_single_camera_sos_amd.omnistereo.pose_est_tools import sequence_windows

WAIT = 5.0   # bound of every wait for an event that must come (a hang fails the test instead of stalling the suite)


class FakeEngine(object):
    """The calls sequence_windows makes on a pipeline.SequenceEngine.  A frame is a string; stage_host copies frames to
    "pinned" buffer b, upload_staged / enqueue_staged copy them to "device" buffer b (enqueue_staged only when no upload of
    that many frames is pending, as _SequenceBase.enqueue_staged), collect returns the device frames of the pending window
    as the records.  A stale call therefore shows twice: in the log, under the run that was current when it came, and in
    the records, as frames of another run."""

    def __init__(self, early_upload=True, enqueue_ahead=True):
        self.early_upload, self.enqueue_ahead = early_upload, enqueue_ahead
        self.run = 0
        self.log = []
        self.pinned, self.device = [[], []], [[], []]
        self.holds = {}    # number of a stage_host call (1, 2, ... over the engine's life) -> (entered, gate) events
        self.n_stage = 0
        self.reset()

    def reset(self):
        self.run += 1
        self._up_pending = [0, 0]
        self._pending = None
        self.stage_s = dict(stage_to_pinned=0.0)

    def _log(self, *call):
        self.log.append((self.run, threading.current_thread().name) + call)

    def stage_host(self, images, buf):
        self.n_stage += 1
        hold = self.holds.get(self.n_stage)
        if hold is not None:
            hold[0].set()
            hold[1].wait(WAIT)
        self.pinned[buf] = list(images)
        self._log("stage_host", buf, tuple(images))

    def upload_staged(self, buf, n):
        self.device[buf] = self.pinned[buf][:n]
        self._up_pending[buf] = n
        self._log("upload_staged", buf, n)

    def enqueue_staged(self, buf, n):
        assert self._pending is None and 0 < n
        if self._up_pending[buf] != n:
            self.device[buf] = self.pinned[buf][:n]
        self._up_pending[buf] = 0
        self._pending = list(self.device[buf][:n])
        self._log("enqueue_staged", buf, n)

    def collect(self):
        p, self._pending = self._pending, None
        self._log("collect", len(p))
        return [dict(frame=f) for f in p]

    def calls(self, run):
        """The calls of `run`, per thread: (consumer's, staging thread's) -- each in a fixed order whatever the timing."""
        mine = [e[1:] for e in self.log if e[0] == run]
        return [e[1:] for e in mine if e[0] != "sosvo-stage"], [e[1:] for e in mine if e[0] == "sosvo-stage"]


class StopOpensGate(threading.Event):
    """The generator's stop event: setting it also opens `gate`, so a staging thread held inside the engine runs on once
    the run has been ended, and not before."""

    def __init__(self, gate):
        threading.Event.__init__(self)
        self.gate = gate

    def set(self):
        threading.Event.set(self)
        self.gate.set()


def _source(name, n, fail_at=None, error=None, block_at=None, entered=None, release=None):
    for i in range(n):
        if i == block_at:
            entered.set()
            release.wait(WAIT)
        if i == fail_at:
            raise error
        yield i, "%s%d" % (name, i), None


def _images(chunk):
    return [item[1] for item in chunk]


def _windows(eng, it, W, stop=None):
    return sequence_windows(it, eng, W, _images, dict(window_s=0.0, windows=0), stop=stop)


def _record(item):
    return item[0], item[1], item[3]["frame"], item[4]


def _stage_threads(before=()):
    return [t for t in threading.enumerate() if t.name == "sosvo-stage" and t not in before]


def _join_all(threads, timeout):
    for t in threads:
        t.join(timeout)


@pytest.mark.parametrize("end", ["close", "consumer_raises"])
def test_ending_a_run_while_the_thread_stages_the_next_window(end):
    """The run ends after its first frame while the staging thread is inside stage_host with window 2.  The copy in flight
    completes before the generator's close() returns; after that, the thread is gone and nothing more reaches the engine:
    no upload of that window, no later window."""
    before = set(_stage_threads())
    eng = FakeEngine(early_upload=True)
    entered, gate = threading.Event(), threading.Event()
    eng.holds[2] = (entered, gate)          # (call 1: window 1, staged by the caller; call 2: the thread's first window)
    gen = _windows(eng, _source("a", 12), 4, stop=StopOpensGate(gate))
    assert _record(next(gen)) == (0, "a0", "a0", 0)
    assert entered.wait(WAIT)
    if end == "close":
        gen.close()
    else:
        error = RuntimeError("the tracker failed")
        with pytest.raises(RuntimeError) as info:
            with contextlib.closing(gen):
                next(gen)
                raise error
        assert info.value is error
    n_log = len(eng.log)
    alive = _stage_threads(before)
    _join_all(alive, WAIT)                  # (whatever a thread left running could still do)
    assert not alive, "the staging thread outlives close()"
    assert eng.log[n_log:] == [], "calls after close(): %r" % (eng.log[n_log:],)
    assert not [e for e in eng.log if e[2] == "upload_staged"], eng.log
    assert not [e for e in eng.log if e[2] == "stage_host" and "a8" in e[4]], eng.log


@pytest.mark.parametrize("W,fail_at", [(4, 6), (4, 4), (8, 6), (1, 3), (4, 0)])
def test_a_failing_source_ends_the_run_after_the_frames_read_before_it(W, fail_at):
    """The source raises while a window is read: every frame read before the failure is yielded (with its record), then
    the source's exception itself reaches the caller, and no staging thread is left."""
    before = set(_stage_threads())
    eng = FakeEngine()
    error = OSError("cannot read frame %d" % fail_at)
    got = []
    with pytest.raises(OSError) as info:
        for item in _windows(eng, _source("a", 12, fail_at=fail_at, error=error), W):
            got.append(_record(item))
    assert info.value is error
    assert got == [(i, "a%d" % i, "a%d" % i, i) for i in range(fail_at)]
    alive = _stage_threads(before)
    _join_all(alive, WAIT)
    assert not alive


@pytest.mark.parametrize("W", [4, 1])
def test_closing_while_the_source_blocks(W):
    """A live source blocks in the middle of the sequence (the staging thread waits in it for the next window).  close()
    returns without waiting for the source; once the source returns, the thread ends within a bounded time without
    staging what it read."""
    before = set(_stage_threads())
    eng = FakeEngine()
    entered, release = threading.Event(), threading.Event()
    gen = _windows(eng, _source("a", 3 * W, block_at=2 * W, entered=entered, release=release), W)
    next(gen)
    assert entered.wait(WAIT)          # (the thread staged window 2 and waits for the first frame of window 3)
    closer = threading.Thread(target=gen.close)
    closer.start()
    closer.join(WAIT)
    try:
        assert not closer.is_alive(), "close() waits for a blocked source"
        n_log = len(eng.log)
        alive = _stage_threads(before)
    finally:
        release.set()
    _join_all(alive, 1.0)
    assert not [t for t in alive if t.is_alive()], "the staging thread survives its source"
    assert eng.log[n_log:] == [], "calls after close(): %r" % (eng.log[n_log:],)
    assert not [e for e in eng.log if e[2] == "stage_host" and "a%d" % (2 * W) in e[4]]


def _run(eng, name, n, W):
    return [_record(item) for item in _windows(eng, _source(name, n), W)]


@pytest.mark.parametrize("early_upload", [True, False])
@pytest.mark.parametrize("enqueue_ahead", [True, False])
@pytest.mark.parametrize("abort", ["in_stage_host", "in_source"])
def test_an_engine_reused_after_an_aborted_run(abort, enqueue_ahead, early_upload):
    """Run 1 is aborted after its first frame -- its staging thread held inside stage_host, or waiting in a blocking
    source that returns only once run 2 is under way -- and run 2 goes through the same engine after reset().  Run 2's
    calls (per thread, in order) and records are those of the same run on a fresh engine."""
    W, n2 = 4, 19
    before = set(_stage_threads())
    eng = FakeEngine(early_upload=early_upload, enqueue_ahead=enqueue_ahead)
    entered, gate = threading.Event(), threading.Event()
    if abort == "in_stage_host":
        eng.holds[2] = (entered, gate)
        src, stop = _source("a", 12), StopOpensGate(gate)
    else:
        src, stop = _source("a", 12, block_at=2 * W, entered=entered, release=gate), None
    gen = _windows(eng, src, W, stop=stop)
    next(gen)
    assert entered.wait(WAIT)
    try:
        gen.close()
        stale = _stage_threads(before)
        eng.reset()
        gen2 = _windows(eng, _source("b", n2), W)
        records = [_record(next(gen2))]
    finally:
        gate.set()                 # (in_source: run 1's source returns while run 2 is under way)
    _join_all(stale, WAIT)
    records += [_record(item) for item in gen2]
    fresh = FakeEngine(early_upload=early_upload, enqueue_ahead=enqueue_ahead)
    assert records == _run(fresh, "b", n2, W) == [(i, "b%d" % i, "b%d" % i, i) for i in range(n2)]
    assert eng.calls(2) == fresh.calls(1)
    assert not [e for e in eng.log if e[0] == 2 and any(str(f).startswith("a") for f in e[4:] if isinstance(f, tuple))]
    _join_all(_stage_threads(before), WAIT)
