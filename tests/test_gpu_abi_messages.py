"""GPU (a context is created; nothing is launched): the stage entry points whose hosts share one body or one set of checks
-- geometry.hip's six assemble entry points, the two gray pyramids, sosvo_track_lk, sosvo_refine_stereo_lk, the gated /
gated-cyclic / ratio matchers, the dense four -- answer every wrong argument with the status and the message, character for
character and with the public function's name in front, that they gave before their hosts were merged.
scripts/record_abi_messages.py makes the raw ctypes calls (one argument wrong per case, two where the order of the checks is
pinned, and the empty input that returns SOSVO_OK early); tests/golden/abi_messages_parent.json holds what the parent commit's
library answered, written by that script from that commit's build.  Here every case is asked again and compared."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_messages_parent.json")))
ENTRY_POINTS = sorted({g[0] for g in GOLDEN})


@pytest.fixture(scope="module")
def answers():
    spec = importlib.util.spec_from_file_location("record_abi_messages", os.path.join(ROOT, "scripts", "record_abi_messages.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return json.loads(json.dumps(mod.record()))


# the distinct messages each entry point's checks hold, counted in the sources (geometry.hip, lk.hip, match.hip, dense.hip,
# dense_speckle.hip): the recorded table has a case for each
MESSAGES = {"sosvo_stereo_assemble": 4, "sosvo_stereo_assemble_slots": 4, "sosvo_f2f_assemble": 3, "sosvo_f2f_assemble_cyclic": 4,
            "sosvo_f2f_assemble_tracked": 3, "sosvo_f2f_assemble_tracked_cyclic": 4, "sosvo_gray_pyramid": 3, "sosvo_gray_pyramid_cyclic": 4,
            "sosvo_track_lk": 13, "sosvo_refine_stereo_lk": 5, "sosvo_match_hamming_gated": 9, "sosvo_match_hamming_gated_cyclic": 10,
            "sosvo_match_hamming_ratio": 14, "sosvo_census_9x7": 4, "sosvo_dense_stereo": 7, "sosvo_dense_triangulate": 4,
            "sosvo_dense_speckle": 6}


def test_the_recorded_table_covers_every_entry_point_and_its_messages():
    assert ENTRY_POINTS == sorted(MESSAGES)
    refused = [g for g in GOLDEN if g[2] != 0]
    assert len(GOLDEN) == 328 and len(refused) == 296 and all(g[2] == -1 for g in refused)      # SOSVO_ERR_ARG, never a HIP error
    assert all(g[3].startswith(g[0] + ": ") for g in refused) and all(g[3] == "" for g in GOLDEN if g[2] == 0)
    assert {e: len({g[3] for g in refused if g[0] == e}) for e in ENTRY_POINTS} == MESSAGES
    # every entry point that has an empty input returned SOSVO_OK on it (the dense four have none)
    assert {g[0] for g in GOLDEN if g[1] == "empty" and g[2] == 0} == {e for e in ENTRY_POINTS if "dense" not in e and "census" not in e}


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_every_answer_is_what_the_parent_commit_gave(answers, entry):
    want = [g for g in GOLDEN if g[0] == entry]
    got = [a for a in answers if a[0] == entry]
    assert [g[:2] for g in got] == [w[:2] for w in want]      # the same cases, in the same order
    differ = [(g, w) for g, w in zip(got, want) if g != w]
    assert not differ, "%d of %d cases differ, the first: %s" % (len(differ), len(want), differ[0])
