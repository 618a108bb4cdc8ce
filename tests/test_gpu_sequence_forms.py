"""GPU: the two forms of every sequence call are one operation, in both families -- ..._front_end by first slot against
..._front_end_slots by table, ..._copy_slot against ..._copy_slots, ..._track with a scalar seed against ..._track_seeds.

Two zero-filled workspaces of one shape, A driven through the single forms and B through the list forms, must end up with
the same counts in every slot and return the same tracking records, row for row and bit for bit: a frame record is a
function of its image, a tracking record of (reference record, current record, seed), whichever call computes or moves it.

Shapes: three rendered frames and an all-black one (an EMPTY record: count 0) at 480 x 640; lanes = 3, window = 6, so
cfg.n_pairs = 18 and the store has 39 slots; omnistereo: 300 features, kp_cap 320, frame_cap 1024.  The frames go to slots 5 .. 8 (8 is
the black one), copies to slots 20 and 21.  17 pairs is beyond the 16 that travel as kernel arguments: the lists are copied
to the device.

The RGB-D family runs at kp_cap = 320 too: up to 1024 the GFT detector keeps 4096 candidates and a whole image has more,
but the kept ones are the 4096 strongest (include/sosvo.h, sosvo_detect_gft, status bit 0), so the records are a function
of the image there as well.  (Before that rule the slots went to whichever waves came first, and the same front-end call
twice on zero-filled workspaces differed in 7 to 48 KB of its keypoints and records.)  Its other cases use the family's
default keypoint capacity (1088: the whole-image variant), once with the 300 features and frame_cap = 1024 of the omni
case and once with 1000 features.

Sizes of the records.  The copy kernel's grid takes 4 x 256 eight-byte words of a field in one pass.  The omni records
here hold 767, 733 and 733 entries: more than one chunk of 256 in every field, and three passes of the stride loop in the
fields of 3 and 4 words per entry.  RGB-D records of 300 features CANNOT exceed 256 entries: of 300 corners, those within
31 pixels of the border get no descriptor (21 % of the image) and 5 % of the pixels have no depth reading (241, 247 and
231 remain); that case runs without the "more than 256" precondition and the one with 1000 features (793, 797 and 787
entries) has it.
A record of more than 1024 ENTRIES, which would take the one-word fields into a second pass too, was tried with
num_of_features = 1500, kp_cap = frame_cap = 2048 on the same rendered omni frames: the counts stayed 767 and 733, so no
synthetic frame gets there and there is no such case."""
import numpy as np
import pytest
import torch

from vo_single_camera_sos_amd import synthetic
from vo_single_camera_sos_amd.frontend import DeviceImageModel
from vo_single_camera_sos_amd.omnistereo.gum import synthetic_gums
from vo_single_camera_sos_amd.omnistereo.panorama import Panorama
from vo_single_camera_sos_amd.pipeline import MultiSequenceEngine, RGBDCamConfig, RGBDMultiSequenceEngine, RigConfig

pytestmark = pytest.mark.gpu

SHAPE = dict(num_of_features=300, kp_cap=320, frame_cap=1024)


class _Omni(object):
    """The omnistereo family's calls on workspace `ws`; images: (omni,)."""

    def __init__(self, ctx, **shape):
        gs = synthetic_gums()
        for m in (gs.top_model, gs.bot_model):
            m.panorama = Panorama(m, width=1200)
        gs.make_annulus_masks((480, 640))
        pano = gs.top_model.panorama
        geo = (pano.cols, pano.rows, pano.pixel_size, pano.cyl_height_max)
        rig = RigConfig(pano_top=geo, pano_bot=geo, F_top=gs.top_model.F[:3, 0], F_bot=gs.bot_model.F[:3, 0], min_range=500.0,
                        max_range=7000.0, stereo_min_disp=1.0, stereo_max_hdiff=2.5, f2f_max_hdiff=0.125 * 0.5 * pano.cols,
                        pct_good_matches=1.0)
        room, rng = synthetic.Room(seed=61), np.random.default_rng(62)
        frames = np.stack([synthetic.render_omni(gs, room, R, t, 2.0, rng)
                           for R, t in synthetic.trajectory(3, 61, max_t=40.0, max_deg=2.0)])
        self.ctx, self.model = ctx, DeviceImageModel(ctx, gs, (480, 640))
        self.eng = e = MultiSequenceEngine(ctx, self.model, rig, lanes=3, window=6, **shape)
        self.images = (torch.from_numpy(np.concatenate([frames, np.zeros_like(frames[:1])])).to(ctx.device),)
        self.shape = (e.cfg, e.window, e.slots)

    def _fe(self, call, ws, where):
        m = self.model
        call(self.eng.rig, *self.shape, *self.images, where, m.unwrap_table, m.mask_bits, m.pattern, ws)

    def front_end(self, ws, first_slot):
        self._fe(self.ctx.sequence_front_end, ws, first_slot)

    def front_end_slots(self, ws, table):
        self._fe(self.ctx.sequence_front_end_slots, ws, table)

    def track(self, ws, ref, cur, seed, out):
        self.ctx.sequence_track(self.eng.rig, *self.shape, ref, cur, seed, ws, out)

    def track_seeds(self, ws, ref, cur, seeds, out):
        self.ctx.sequence_track_seeds(self.eng.rig, *self.shape, ref, cur, seeds, ws, out)

    def copy_slot(self, ws, src, dst):
        self.ctx.sequence_copy_slot(*self.shape, src, dst, ws)

    def copy_slots(self, ws, src, dst):
        self.ctx.sequence_copy_slots(*self.shape, src, dst, ws)

    def counts(self, ws):
        return self.ctx.sequence_frame_counts(*self.shape, 0, self.eng.slots, ws)


class _RGBD(object):
    """The RGB-D family's; images: (bgr, depth), the black frame has no depth reading either."""

    def __init__(self, ctx, **shape):
        cam = RGBDCamConfig(fx=554.256258, fy=554.256258, center_x=319.5, center_y=239.5, depth_is_Z=False, min_range=0.8,
                            max_range=7.0)
        bgr, depth, _ = synthetic.make_rgbd_sequence(3, seed=41, max_t=40.0, max_deg=2.0, depth_is_Z=False)
        depth = np.ascontiguousarray(depth, dtype=np.float32)
        self.ctx = ctx
        self.eng = e = RGBDMultiSequenceEngine(ctx, cam, lanes=3, window=6, **shape)
        self.images = (torch.from_numpy(np.concatenate([bgr, np.zeros_like(bgr[:1])])).to(ctx.device),
                       torch.from_numpy(np.concatenate([depth, np.zeros_like(depth[:1])])).to(ctx.device))
        self.shape = (e.cfg, e.window, e.slots)

    def _fe(self, call, ws, where):
        e = self.eng
        call(e.cam, *self.shape, *self.images, where, e.mask_bits, e.pattern, ws)

    def front_end(self, ws, first_slot):
        self._fe(self.ctx.rgbd_sequence_front_end, ws, first_slot)

    def front_end_slots(self, ws, table):
        self._fe(self.ctx.rgbd_sequence_front_end_slots, ws, table)

    def track(self, ws, ref, cur, seed, out):
        self.ctx.rgbd_sequence_track(*self.shape, ref, cur, seed, ws, out)

    def track_seeds(self, ws, ref, cur, seeds, out):
        self.ctx.rgbd_sequence_track_seeds(*self.shape, ref, cur, seeds, ws, out)

    def copy_slot(self, ws, src, dst):
        self.ctx.rgbd_sequence_copy_slot(*self.shape, src, dst, ws)

    def copy_slots(self, ws, src, dst):
        self.ctx.rgbd_sequence_copy_slots(*self.shape, src, dst, ws)

    def counts(self, ws):
        return self.ctx.rgbd_sequence_frame_counts(*self.shape, 0, self.eng.slots, ws)


@pytest.mark.parametrize("family,shape,beyond_a_chunk", [(_Omni, SHAPE, True), (_RGBD, dict(SHAPE, kp_cap=None), False),
                                                         (_RGBD, dict(num_of_features=1000), True), (_RGBD, SHAPE, False)])
def test_single_and_list_forms_are_one_operation(ctx, family, shape, beyond_a_chunk):
    f = family(ctx, **shape)
    assert f.eng.cfg.n_pairs == 18 and f.eng.slots == 39
    A, B = torch.zeros_like(f.eng.workspace), torch.zeros_like(f.eng.workspace)
    # ---- front end: by first slot, by table
    f.front_end(A, 5)
    f.front_end_slots(B, [5, 6, 7, 8])
    counts = f.counts(A)
    print("counts of slots 5 .. 8:", counts[5:9])
    assert counts == f.counts(B)
    assert counts[8] == 0 and all(c == 0 for i, c in enumerate(counts) if not 5 <= i <= 8)
    assert max(counts) > 256 or not beyond_a_chunk, "the copy of such a record takes more than one chunk of 256 entries"
    # ---- copy: two single calls (the second one of an empty record), one list call
    f.copy_slot(A, 5, 20)
    f.copy_slot(A, 8, 21)
    f.copy_slots(B, [5, 8], [20, 21])
    copied = f.counts(A)
    assert copied == f.counts(B)
    assert copied[20] == counts[5] and copied[21] == 0 and copied[:20] == counts[:20] and copied[22:] == counts[22:]
    f.copy_slot(A, 6, 6)                      # a slot onto itself: no error, nothing changes (B never sees such a call)
    assert f.counts(A) == copied
    # ---- track: pair i of the scalar form samples with seed + i
    out_a, out_b = (torch.zeros((18, 16), dtype=torch.float64, device=ctx.device) for _ in range(2))
    live = [5, 6, 7, 8, 20, 21]
    few = ([5, 20, 6], [7, 7, 5])
    many = ([live[i % 6] for i in range(17)], [live[(i + 1 + i // 6) % 6] for i in range(17)])   # (slots repeat, ref != cur)
    for ref, cur in (few, many):
        for s in (3, 2 ** 35):
            n = len(ref)
            f.track(A, ref, cur, s, out_a)
            f.track_seeds(B, ref, cur, [s + i for i in range(n)], out_b)
            a, b = out_a[:n].cpu().numpy(), out_b[:n].cpu().numpy()
            assert np.array_equal(a, b), (n, s)
            assert a[0, 14] == 0 and a[0, 12] > 30, "the first pair (two rendered frames) is tracked"
    # the copy is the original: (5, 7) and (20, 7) with ONE seed give one record (in a call they are rows i and i + 1 and
    # sample with different seeds, so each gets a call of its own in the scalar form)
    for s in (3, 2 ** 35):
        f.track(A, [5], [7], s, out_a)
        f.track(A, [20], [7], s, out_a[1:])
        f.track_seeds(B, [5, 20], [7, 7], [s, s], out_b)
        a, b = out_a[:2].cpu().numpy(), out_b[:2].cpu().numpy()
        assert np.array_equal(a[0], a[1]) and np.array_equal(a, b) and a[0, 14] == 0

