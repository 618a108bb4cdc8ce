"""CPU: device.Context against a recording of itself.  tests/golden/context_calls_parent.json was written by
scripts/record_context_calls.py from device.py as it stood before its buffer records were folded into one description each,
unchanged, and no later commit touches it: for some two thousand calls -- every public method with its optional outputs
left out and supplied, every switch, and one refused call per rule (1639 of them, which say exactly what _check says for
the rule that was broken, as a count in their plain call's record) -- it holds the ordered checks (name, dtype, shape,
ndim), the ordered library calls with every argument decoded by the parameter names of include/sosvo.h, what each buffer the
method allocates holds, and the structure of what comes back; or the type and text of the exception.  The sweep is run
again here, on host tensors with a recorder in place of the library (libsosvo.so is never loaded), and must give the same
bytes."""
import importlib.util
import json
import os
import re

import pytest

from vo_single_camera_sos_amd import _lib, device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def recorder():
    spec = importlib.util.spec_from_file_location("record_context_calls", os.path.join(ROOT, "scripts", "record_context_calls.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded(recorder):
    loaded = _lib._lib
    records = recorder.sweep()
    assert _lib._lib is loaded, "the sweep loaded libsosvo.so"
    return records


@pytest.fixture(scope="module")
def golden(recorder):
    return open(recorder.GOLDEN).read()


def test_every_case_gives_what_the_parent_gave(recorder, recorded, golden):
    want = {r["id"]: r for r in json.loads(golden)}
    got = {r["id"]: r for r in json.loads(recorder.text(recorded))}     # (through JSON: tuples are lists in both)
    assert len(got) == len(recorded), "case ids are not unique"
    assert sorted(got) == sorted(want)
    differing = [cid for cid in want if got[cid] != want[cid]]
    assert not differing, "%d cases differ, the first: %s\n  parent: %s\n  now:    %s" % (
        len(differing), differing[0], json.dumps(want[differing[0]]), json.dumps(got[differing[0]]))


def test_the_sweep_reproduces_the_committed_file_byte_for_byte(recorder, recorded, golden):
    assert recorder.text(recorded) == golden
    assert len(golden) < 512 * 1024 and max(len(line) for line in golden.split("\n")) < 8192       # compact: one case per line


def test_the_sweep_leaves_the_module_as_it_was(recorded):
    import torch
    assert device.torch is torch and device.ctypes.__name__ == "ctypes" and device._check.__module__ == device.__name__
    assert torch.zeros(1).is_cuda is False


def test_every_public_method_is_called_plain_and_every_entry_point_is_reached(recorded):
    called = {r["id"].split("/")[0] for r in recorded if "calls" in r}
    public = {name for name, v in vars(device.Context).items() if callable(v) and not name.startswith("_")} - {"close"}
    assert public <= called, sorted(public - called)
    entries = {c[0] for r in recorded for c in r.get("calls", ())}
    # what only __init__, close and the real _call reach, and what has no method of Context
    plumbing = {"sosvo_create", "sosvo_destroy", "sosvo_last_error", "sosvo_abi_version", "sosvo_orb_bit_pattern_31",
                "sosvo_describe_orb", "sosvo_subpix_weights", "sosvo_gray_pyramid_bytes"}
    assert entries == set(_lib.SIGNATURES) - plumbing


def test_no_argument_is_left_undecoded_and_every_rule_speaks(recorded):
    text = json.dumps(recorded)
    assert "unknown" not in text
    refused = [r for r in recorded if "raises" in r]
    # the generated refusals: those that say exactly what _check says for the broken rule are counted in their plain call,
    # the others (an earlier rule speaks, or an attribute of the non-tensor is read first) are records of their own
    by_rule, own = sum(r.get("by_rule", 0) for r in recorded), [r for r in refused if "!" in r["id"]]
    assert by_rule > 1500 and len(own) >= 50 and all("by_rule" not in r for r in refused)
    # the hand-written raises of device.py: every message of the file is among the refusals (the two of __init__ and the
    # residency rule aside)
    source = open(device.__file__).read()
    messages = re.findall(r'raise (?:SosvoError|ValueError)\(\s*"([^"%]{12,})', source)
    assert len(messages) >= 25
    spoken = " ".join(r["raises"][1] for r in refused)
    silent = [m for m in messages if m not in spoken and "no GPU visible" not in m and "sosvo_create failed" not in m]
    assert not silent, silent


def test_the_sweep_executes_every_line_but_the_plumbing_that_needs_a_device(recorder):
    """The condition under which device.py may be rewritten against the recording: a line the sweep does not reach is not
    pinned.  Left out: __init__, close, __del__, the real _call, and the residency branch of _check."""
    missed = recorder.uncovered_lines()
    outside = {line: fn for line, fn in missed.items() if fn not in ("Context.__init__", "Context.close", "Context.__del__", "Context._call", "_check")}
    assert not outside, outside
    source = open(device.__file__).read().split("\n")
    assert [source[line - 1].strip() for line, fn in missed.items() if fn == "_check"] == \
        ['raise SosvoError("%s: must live on the GPU" % name)']
