"""CPU: the one Python matching step and its options value.  Context.match_1nn (the twin of match_1nn in pipeline.hip) and
the two forms built on it, match_1nn_slots and match_1nn_two_launch, are driven with host tensors and a recorder in place of
the library: what is asserted is WHICH entry points are called, in which order, with which scalars and buffers -- stated
here by rule (ratio -> sosvo_match_hamming_ratio, else gate -> sosvo_match_hamming_gated, else sosvo_match_hamming), the
arguments decoded by the names of the prototypes in include/sosvo.h.  No device call is made.  Then _lib.MatchOptions."""
import itertools
from types import SimpleNamespace

import pytest
import torch
from sosvo_header import parameter_names as _parameter_names

from vo_single_camera_sos_amd import _lib, device
from vo_single_camera_sos_amd._lib import MatchOptions
from vo_single_camera_sos_amd.device import Context

PLAIN, GATED, RATIO, CROSS = ("sosvo_match_hamming", "sosvo_match_hamming_gated", "sosvo_match_hamming_ratio",
                              "sosvo_cross_check_matches")
GATE = (1.0, 2.5, 80)                      # (min_dv, max_du, max_distance)
COMBOS = list(itertools.product((0, 48), (None, GATE), (False, True)))      # ratio in 64ths, gate, cross-check
IDS = ["%s-%s-%s" % ("ratio" if r else "noratio", "gate" if g else "nogate", "cc" if cc else "nocc") for r, g, cc in COMBOS]


@pytest.fixture
def ctx(monkeypatch):
    """A Context without a device: the tensors live on the host, so the residency checks are off, and _call records
    (entry, {parameter name: value}) with pointers as integers (None: NULL)."""
    monkeypatch.setattr(device, "_check", lambda t, *args, **kwargs: t)
    c = Context.__new__(Context)
    c._lib = SimpleNamespace(**{name: name for name in _lib.SIGNATURES})
    c.calls = []

    def record(entry, *args):
        names = _parameter_names(entry)
        assert len(args) == len(names), entry
        c.calls.append((entry, {n: getattr(a, "value", a) for n, a in zip(names, args)}))
    c._call = record
    return c


def _u8(*shape):
    return torch.zeros(shape, dtype=torch.uint8)


def _problem(P=3, Sq=5, St=7):
    """P problems of Sq queries and St trains: descriptors, positions, counts."""
    return SimpleNamespace(P=P, Sq=Sq, St=St, q=_u8(P, Sq, 32), t=_u8(P, St, 32), qp=torch.zeros((P, Sq, 2)),
                           tp=torch.zeros((P, St, 2)), nq=torch.zeros(P, dtype=torch.int32), nt=torch.zeros(P, dtype=torch.int32))


def _keys(P, S):
    return torch.zeros((P, S, 1), dtype=torch.uint32)


def _entry(ratio, gate):
    return RATIO if ratio else GATED if gate else PLAIN


def _search(ratio, gate, q, t, qp, tp, nq, nt, q_slot, t_slot, nprob, n_forward, Sq, St, keys, rivals):
    """The one library call of a best-match search, by rule."""
    want = dict(q_desc=q.data_ptr(), t_desc=t.data_ptr(), nq=nq.data_ptr(), nt=nt.data_ptr(),
                q_slot=None if q_slot is None else q_slot.data_ptr(), t_slot=None if t_slot is None else t_slot.data_ptr(),
                nprob=nprob, q_stride=Sq, t_stride=St, keys=keys.data_ptr())
    if not (ratio or gate):
        return PLAIN, dict(want, k=1)                        # (the plain entry has no n_forward)
    want.update(q_pos=qp.data_ptr() if gate else None, t_pos=tp.data_ptr() if gate else None, n_forward=n_forward,
                min_dv=gate[0] if gate else -1.0, max_du=gate[1] if gate else 0.0,
                max_distance=256 if not gate or gate[2] is None else gate[2])
    if ratio:
        want.update(ratio_64ths=ratio, rivals=rivals.data_ptr())
    return _entry(ratio, gate), want


@pytest.mark.parametrize("ratio,gate,cc", COMBOS, ids=IDS)
def test_match_1nn_makes_exactly_one_call_of_the_entry_the_rule_names(ctx, ratio, gate, cc):
    s = _problem()
    keys, rivals = _keys(s.P, s.Sq), _keys(s.P, s.Sq)
    n_forward = 2 if cc else None                            # (None: every problem is a forward one)
    got = ctx.match_1nn(s.q, s.t, s.nq, s.nt, ratio_64ths=ratio, rivals=rivals, gate=gate, q_pos=s.qp, t_pos=s.tp, keys=keys,
                        n_forward=n_forward)
    assert got is keys and len(ctx.calls) == 1
    entry, args = ctx.calls[0]
    assert entry == _entry(ratio, gate)
    assert (entry, args) == _search(ratio, gate, s.q, s.t, s.qp, s.tp, s.nq, s.nt, None, None, s.P,
                                    s.P if n_forward is None else n_forward, s.Sq, s.St, keys, rivals)
    assert ("n_forward" in args) == (entry != PLAIN)
    if entry != PLAIN:
        assert (args["min_dv"], args["max_du"], args["max_distance"]) == ((1.0, 2.5, 80) if gate else (-1.0, 0.0, 256))
    if entry == RATIO:
        assert args["ratio_64ths"] == 48


def test_match_1nn_passes_no_cap_as_256_and_allocates_what_it_is_not_given(ctx):
    s = _problem()
    keys = ctx.match_1nn(s.q, s.t, s.nq, s.nt, gate=(-1.0, 37.5, None), q_pos=s.qp, t_pos=s.tp)
    assert tuple(keys.shape) == (s.P, s.Sq, 1) and keys.dtype == torch.uint32
    (entry, args), = ctx.calls
    assert entry == GATED and (args["min_dv"], args["max_du"], args["max_distance"], args["n_forward"]) == (-1.0, 37.5, 256, s.P)
    assert args["keys"] == keys.data_ptr()


@pytest.mark.parametrize("ratio,gate,cc", COMBOS, ids=IDS)
def test_the_two_launch_form_issues_the_forward_search_then_the_swapped_one_then_the_filter(ctx, ratio, gate, cc):
    s = _problem()
    keys, rev, rivals = _keys(s.P, s.Sq), _keys(s.P, s.St), _keys(s.P, s.Sq)
    got = ctx.match_1nn_two_launch(s.q, s.t, s.nq, s.nt, cross_check=cc, keys_rev=rev, ratio_64ths=ratio, rivals=rivals, gate=gate,
                                   q_pos=s.qp, t_pos=s.tp, keys=keys)
    assert got is keys
    want = [_search(ratio, gate, s.q, s.t, s.qp, s.tp, s.nq, s.nt, None, None, s.P, s.P, s.Sq, s.St, keys, rivals)]
    if cc:
        # roles and positions swapped, every problem reversed (n_forward = 0), never the ratio rule; then the mutual filter
        want.append(_search(0, gate, s.t, s.q, s.tp, s.qp, s.nt, s.nq, None, None, s.P, 0, s.St, s.Sq, rev, None))
        want.append((CROSS, dict(keys_fwd=keys.data_ptr(), keys_rev=rev.data_ptr(), nq=s.nq.data_ptr(), nt=s.nt.data_ptr(),
                                 q_slot=None, t_slot=None, nprob=s.P, q_stride=s.Sq, t_stride=s.St, keys_out=keys.data_ptr())))
    assert len(ctx.calls) == len(want) == (3 if cc else 1)
    for (entry, args), (want_entry, want_args) in zip(ctx.calls, want):
        args.pop("n_kept", None)                             # (allocated by the call)
        assert (entry, args) == (want_entry, want_args)
    if cc:
        assert ctx.calls[1][0] != RATIO and ctx.calls[1][0] == (GATED if gate else PLAIN)


@pytest.mark.parametrize("ratio,gate,cc", COMBOS, ids=IDS)
def test_the_slot_form_issues_one_search_with_the_swapped_problems_behind_the_forward_ones(ctx, ratio, gate, cc):
    F, S, blocks = 3, 6, 8                                   # forward problems, rows per block, blocks
    d, pos, n = _u8(blocks, S, 32), torch.zeros((blocks, S, 2)), torch.zeros(blocks, dtype=torch.int32)
    P = 2 * F if cc else F
    q_slot, t_slot = torch.zeros(P, dtype=torch.int32), torch.zeros(P, dtype=torch.int32)
    keys, rivals = _keys(P, S), _keys(P, S)
    fwd = ctx.match_1nn_slots(d, pos, n, q_slot, t_slot, keys, F, ratio_64ths=ratio, rivals=rivals, gate=gate)
    assert fwd.data_ptr() == keys.data_ptr() and tuple(fwd.shape) == (F, S, 1)
    want = [_search(ratio, gate, d, d, pos, pos, n, n, q_slot, t_slot, P, F, S, S, keys, rivals)]
    if cc:      # the two halves of the one launch: forward keys against the role-swapped problems' keys, in place
        want.append((CROSS, dict(keys_fwd=keys.data_ptr(), keys_rev=keys[F:].data_ptr(), nq=n.data_ptr(), nt=n.data_ptr(),
                                 q_slot=q_slot.data_ptr(), t_slot=t_slot.data_ptr(), nprob=F, q_stride=S, t_stride=S,
                                 keys_out=keys.data_ptr())))
    assert len(ctx.calls) == len(want) == (2 if cc else 1)
    for (entry, args), (want_entry, want_args) in zip(ctx.calls, want):
        args.pop("n_kept", None)
        assert (entry, args) == (want_entry, want_args)
    if _entry(ratio, gate) != PLAIN:
        assert ctx.calls[0][1]["n_forward"] == F


# ---- MatchOptions ---------------------------------------------------------------------------------------------------------------
NAMES = ("cross_check_stereo", "cross_check_f2f", "gated_stereo", "gated_f2f", "gated_max_distance", "ratio_stereo", "ratio_f2f",
         "ratio")


def test_match_options_fields_and_defaults():
    o = MatchOptions()
    assert o._fields == NAMES and tuple(o) == (False, False, False, False, None, False, False, None)
    assert o.flags() == 0 and (o.ratio_64ths_stereo, o.ratio_64ths_f2f) == (0, 0)
    assert MatchOptions(**o._asdict()) == o and hash(o) == hash(MatchOptions())
    with pytest.raises(AttributeError):
        o.ratio = 0.75                                       # immutable


def test_match_options_flags_are_the_or_of_the_three_flag_functions():
    n = 0
    for cs, cf, gs, gf, rs, rf in itertools.product((False, True), repeat=6):
        for cap in (None, 1, 80, 256):
            for ratio in (None, 1 / 64.0, 0.75, 63 / 64.0):
                if (rs or rf) and ratio is None:
                    with pytest.raises(ValueError, match="needs a ratio"):
                        MatchOptions(cs, cf, gs, gf, cap, rs, rf, ratio)
                    continue
                o = MatchOptions(cs, cf, gs, gf, cap, rs, rf, ratio)
                assert o.flags() == (_lib.cross_check_flags(cs, cf) | _lib.gated_flags(gs, gf, cap) | _lib.ratio_flags(rs, rf, ratio))
                r64 = 0 if ratio is None else int(ratio * 64)
                assert (o.ratio_64ths_stereo, o.ratio_64ths_f2f) == (r64 if rs else 0, r64 if rf else 0)
                assert o == MatchOptions(**o._asdict()) and tuple(o) == (cs, cf, gs, gf, cap, rs, rf, ratio)
                n += 1
    assert n == 64 * 16 - 48 * 4


def test_match_options_refuses_with_the_flag_functions_messages():
    for cap in (0, 257, 12.5):
        with pytest.raises(ValueError, match=r"gated_max_distance must be None or an integer in 1 \.\. 256"):
            MatchOptions(gated_f2f=True, gated_max_distance=cap)
    for ratio in (0.7, 0.0, 1.0, 48, "x"):
        with pytest.raises(ValueError, match=r"ratio must be a float in \(0, 1\) with ratio \* 64 an integer"):
            MatchOptions(ratio_stereo=True, ratio=ratio)
    with pytest.raises(ValueError, match="nearest admissible values are 0.6875"):
        MatchOptions(ratio=0.7)                              # (checked even without a switch, as ratio_flags does)
    with pytest.raises(ValueError, match="the ratio test needs a ratio"):
        MatchOptions(ratio_f2f=True)


def test_match_options_keys_distinguish_every_setting():
    seen = {MatchOptions(cs, cf, gs, gf, cap, rs, rf, 0.75 if rs or rf else None)
            for cs, cf, gs, gf, rs, rf in itertools.product((False, True), repeat=6) for cap in (None, 80)}
    assert len(seen) == 128
    assert MatchOptions(ratio_f2f=True, ratio=0.75) != MatchOptions(ratio_f2f=True, ratio=51 / 64.0)


def test_the_rgbd_constructor_takes_the_rgbd_names_only():
    kw = dict(cross_check=True, gated_f2f=True, gated_max_distance=80, ratio_f2f=True, ratio=0.75)
    o = MatchOptions.rgbd(**kw)
    assert o == MatchOptions(False, True, False, True, 80, False, True, 0.75) and o.rgbd_kwargs() == kw
    assert MatchOptions.rgbd() == MatchOptions() and MatchOptions.rgbd(*kw.values()) == o
    assert o.flags() & (_lib.FLAG_CROSS_CHECK_STEREO | _lib.FLAG_GATED_STEREO | _lib.FLAG_RATIO_STEREO) == 0
    for name in ("cross_check_stereo", "gated_stereo", "ratio_stereo", "cross_check_f2f"):
        with pytest.raises(TypeError, match=name):
            MatchOptions.rgbd(**{name: True})
    with pytest.raises(ValueError, match="gated_max_distance"):
        MatchOptions.rgbd(gated_f2f=True, gated_max_distance=0)


def test_from_matchers_follows_the_matchers_and_knows_what_has_no_batched_counterpart():
    from vo_single_camera_sos_amd.omnistereo.camera_models import FeatureMatcher
    fm = lambda **kw: FeatureMatcher("GFT", "BF", 1, **kw)  # noqa: E731
    assert MatchOptions.from_matchers(fm(), fm()) == MatchOptions() == MatchOptions.from_matchers(None, None)
    o = MatchOptions.from_matchers(fm(cross_check=True, gated=True, gated_max_distance=80), fm(ratio=0.75))
    assert o == MatchOptions(cross_check_stereo=True, gated_stereo=True, gated_max_distance=80, ratio_f2f=True, ratio=0.75)
    # cap and ratio of a matcher that is off are no part of the value
    assert MatchOptions.from_matchers(fm(gated_max_distance=64), fm(gated=True)) == MatchOptions(gated_f2f=True)
    assert MatchOptions.from_matchers(None, fm(gated=True, gated_max_distance=64)).rgbd_kwargs()["gated_max_distance"] == 64
    # one cap and one ratio for both matchers
    assert MatchOptions.from_matchers(fm(gated=True, gated_max_distance=64), fm(gated=True, gated_max_distance=80)) is None
    assert MatchOptions.from_matchers(fm(gated=True), fm(gated=True, gated_max_distance=80)) is None
    assert MatchOptions.from_matchers(fm(ratio=0.5), fm(ratio=0.75)) is None
    assert MatchOptions.from_matchers(fm(ratio=0.5), fm(ratio=0.5)) == MatchOptions(ratio_stereo=True, ratio_f2f=True, ratio=0.5)
