"""The inputs of tests/test_gpu_lk_lattice.py, tests/test_gpu_stereo_lk_lattice.py and tests/test_lk_lattice_reference.py, and
their CPU references (tests/reflk.py, reflk_cyclic.py, refstereolk.py, refsubpix.py): host arrays built from fixed seeds, each
case and each reference made once per process and handed out read-only.

A tracker case (TrackCase) is one call of sosvo_track_lk.  `first_round` is how many keypoints of a problem the launch takes
in its first round of the keypoint loop -- rows of the grid times keypoints per wave: 64 x 1 for the whole-wave form (half
6 .. 10), 64 x 4 for the 16-lane form (half 2 .. 5), 16 x 1 and 16 x 4 from 4096 problems on; points at and beyond that index
are the ones a later round tracks.  `live` names the problems a reference has to run (None: all)."""
import numpy as np

import reflk
import reflk_cyclic
import refstereolk
import refsubpix

SENTINEL = np.float32(-123.25)
ST_SENTINEL = 0xA5
MAX_ITER = 10
ROWS, COLS = 96, 128
FB_MAX = 0.5

_made = {}


def _once(key, make):
    if key not in _made:
        _made[key] = make()
    return _made[key]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


def first_round(half, nprob):
    return (16 if nprob >= 4096 else 64) * (4 if half <= 5 else 1)


# ---- starts ------------------------------------------------------------------------------------------------------------------------
def starts(rng, count, cap, rows, cols, other=0, margin=(14, 26), seam=0):
    """count starts in a [cap, 2] table of sentinels: integer and fractional ones `margin` inside the image, anywhere in the image
    and a little outside; and in every run of 16 rows an image corner (row 3), a non-finite start (row 7: skipped) and a start
    just above the first row (row 12: lost), so that whichever round of the keypoint loop takes a run meets all of them.
    seam (cyclic columns): the first `seam` starts sit in the columns on either side of column 0."""
    mx, my = margin
    kp = np.full((cap, 2), SENTINEL, np.float32)
    cols_at_seam = list(range(seam // 2)) + list(range(cols - seam // 2, cols))
    for k in range(count):
        if k < seam:
            kp[k] = cols_at_seam[k], (my + 4 + 2 * k if k % 2 else rng.uniform(my, rows - 1 - my))
        elif k % 16 == 3:
            kp[k] = (0, 0) if (k // 16 + other) % 2 == 0 else (cols - 1, rows - 1)
        elif k % 16 == 7:
            kp[k] = (np.nan, 20) if (k // 16 + other) % 2 else (20, np.inf)
        elif k % 16 == 12:
            kp[k] = cols - 0.4, -0.6
        elif k % 3 == 0:
            kp[k] = rng.integers(mx, cols - mx), rng.integers(my, rows - my)
        elif k % 3 == 1:
            kp[k] = rng.uniform(mx, cols - 1 - mx), rng.uniform(my, rows - 1 - my)
        else:
            kp[k] = rng.uniform(-2, cols + 1), rng.uniform(-2, rows + 1)
    return kp


def guesses(rng, pts):
    """The initial-flow flag's guesses: the starts moved by about a pixel, one of them non-finite."""
    g = (pts + np.float32(1.0) + rng.uniform(-1, 1, pts.shape)).astype(np.float32)
    g[0, 9] = np.nan, 3.0
    return g


# ---- tracker cases -----------------------------------------------------------------------------------------------------------------
class TrackCase:
    def __init__(self, key, gray, levels, half, pts, n, prev_img, next_img, cyclic=False, fb_max=None, guess=None, live=None):
        self.key, self.levels, self.half, self.cyclic, self.fb_max = key, levels, half, cyclic, fb_max
        self.gray, self.pts, self.guess = gray, pts, guess
        self.n, self.prev_img, self.next_img = (np.asarray(a, np.int32) for a in (n, prev_img, next_img))
        self.live = live
        self.nprob, self.cap = pts.shape[:2]
        self.first_round = first_round(half, self.nprob)
        _frozen(*(a for a in (self.gray, self.pts, self.guess, self.n, self.prev_img, self.next_img) if a is not None))

    def sentinels(self):
        """(next, status, err, back) as the device buffers start: the sentinel everywhere (next: the guesses, where given)."""
        shape = (self.nprob, self.cap)
        nxt = np.full(shape + (2,), SENTINEL, np.float32) if self.guess is None else self.guess.copy()
        return (nxt, np.full(shape, ST_SENTINEL, np.uint8), np.full(shape, SENTINEL, np.float32),
                np.full(shape + (2,), SENTINEL, np.float32))

    def __repr__(self):
        return self.key


def _pairs(cyclic, rows=ROWS, cols=COLS):
    """Six images: pair A = images (0, 1), a small shift; pair B = (2, 3), a shift of several pixels; pair C = (4, 5), two
    unrelated textures -- a track between them ends wherever the iteration stops, and the way back ends somewhere else, which is
    what the forward-backward check is there to clear."""
    def make():
        tex = reflk_cyclic.texture if cyclic else reflk.texture
        small = (5.3, -3.6) if cyclic else (1.37, -0.71)            # (cyclic: both signs of a shift that carries points across)
        large = (-5.3, 3.6) if cyclic else (5.3, -3.6)
        return _frozen(np.stack([tex(11, rows, cols), tex(11, rows, cols, small), tex(12, rows, cols), tex(12, rows, cols, large),
                                 tex(13, rows, cols), tex(14, rows, cols)]))
    return _once(("pairs", cyclic, rows, cols), make)


PREV_IMG, NEXT_IMG = (0, 2, 4, 2), (1, 3, 5, 3)          # the lattice: problem 2 tracks between strangers
ROUNDS_PREV, ROUNDS_NEXT = (4, 0, 2, 2), (5, 1, 3, 3)    # later rounds: problem 0, the one with most rows beyond the first, does
CYCLIC_PREV, CYCLIC_NEXT = (0, 4, 2, 2), (1, 5, 3, 3)    # cyclic cells: the lone point of problem 1 does


def _table(seed, counts, cap, rows=ROWS, cols=COLS, **kw):
    rng = np.random.default_rng(seed)
    return np.stack([starts(rng, c, cap, rows, cols, other=p & 1, **kw) for p, c in enumerate(counts)])


# 1(a): every window on every depth
LATTICE_HALVES, LATTICE_LEVELS, LATTICE_COUNTS = tuple(range(2, 11)), (1, 2, 3, 4), (24, 1, 5, 0)


def lattice_case(half, levels, variant=None):
    def make():
        pts = _once("lattice pts", lambda: _frozen(_table(23, LATTICE_COUNTS, 80)))
        guess = guesses(np.random.default_rng(5), pts) if variant == "guess" else None
        return TrackCase("lattice half %d levels %d %s" % (half, levels, variant), _pairs(False), levels, half, pts, LATTICE_COUNTS,
                         PREV_IMG, NEXT_IMG, fb_max=FB_MAX if variant == "fb" else None, guess=guess)
    return _once(("lattice", half, levels, variant), make)


# 1(b): later rounds and a ragged last one
ROUNDS = [(6, 1), (6, 3), (10, 1), (10, 3), (2, 1), (5, 1), (5, 4)]     # (half, levels); each with and without the check
WAVE_COUNTS, GROUP_COUNTS = (80, 65, 64, 0), (300, 257, 256, 1)


def rounds_case(half, levels, fb):
    def make():
        counts, cap = (GROUP_COUNTS, 300) if half <= 5 else (WAVE_COUNTS, 80)
        pts = _once(("rounds pts", cap), lambda: _frozen(_table(29, counts, cap)))
        return TrackCase("rounds half %d levels %d fb %s" % (half, levels, fb), _pairs(False), levels, half, pts, counts, ROUNDS_PREV,
                         ROUNDS_NEXT, fb_max=FB_MAX if fb else None)
    return _once(("rounds", half, levels, fb), make)


# 1(c): the wide grid
WIDE_NPROB, WIDE_CAP, WIDE_LEVELS = 4096, 80, 2
WIDE_LIVE = ((0, 80), (5, 17), (1023, 65), (2048, 1), (2049, 80), (3333, 65), (4000, 17), (4095, 65))     # (problem, count)
WIDE_NO_IMAGE = ((7, -1, 1, 40), (4090, 2, 6, 80))     # (problem, prev_img, next_img, count): an image index off the set


def wide_case(half, cyclic=False):
    def make():
        rng = np.random.default_rng(37)
        pts = np.full((WIDE_NPROB, WIDE_CAP, 2), SENTINEL, np.float32)
        n = np.zeros(WIDE_NPROB, np.int32)
        prev_img = (2 * (np.arange(WIDE_NPROB) & 1)).astype(np.int32)
        next_img = prev_img + 1
        for i, (p, c) in enumerate(WIDE_LIVE):
            pts[p], n[p] = starts(rng, c, WIDE_CAP, ROWS, COLS, other=i & 1, seam=12 if cyclic else 0), c
        for p, a, b, c in WIDE_NO_IMAGE:
            pts[p], n[p], prev_img[p], next_img[p] = starts(rng, c, WIDE_CAP, ROWS, COLS), c, a, b
        return TrackCase("wide half %d cyclic %s" % (half, cyclic), _pairs(cyclic), WIDE_LEVELS, half, pts, n, prev_img, next_img,
                         cyclic=cyclic, live=[p for p, _ in WIDE_LIVE])
    return _once(("wide", half, cyclic), make)


# 1(d): tiny images
TINY_TEXTURED, TINY_FLAT = ((5, 40), (40, 5), (9, 12)), ((1, 70), (70, 1), (1, 1))
TINY_HALVES, TINY_LEVELS, TINY_COUNT = (2, 5, 6, 10), (1, 4), 16


def tiny_case(shape, half, levels):
    def make():
        rows, cols = shape
        gray = _once(("tiny gray", shape), lambda: _frozen(np.stack([reflk.texture(5, rows, cols, lo=3.0, hi=12.0),
                                                                     reflk.texture(5, rows, cols, (0.4, -0.3), lo=3.0, hi=12.0)])))
        pts = _once(("tiny pts", shape), lambda: _frozen(_table(rows + cols, (TINY_COUNT,), TINY_COUNT, rows, cols, margin=(0, 0))))
        return TrackCase("tiny %d x %d half %d levels %d" % (rows, cols, half, levels), gray, levels, half, pts, (TINY_COUNT,), (0,), (1,))
    return _once(("tiny", shape, half, levels), make)


# 1(e): cyclic columns
CYCLIC_CELLS = [(5, 1), (5, 3), (6, 1), (6, 3)]
CYCLIC_COUNTS = (40, 1, 24, 0)
CYCLIC_ROUNDS = [(5, 4, 300, 257), (6, 3, 80, 65)]       # (half, levels, cap, count), with the forward-backward check


def cyclic_case(half, levels):
    def make():
        pts = _once("cyclic pts", lambda: _frozen(_table(31, CYCLIC_COUNTS, 80, margin=(0, 26), seam=24)))
        return TrackCase("cyclic half %d levels %d" % (half, levels), _pairs(True), levels, half, pts, CYCLIC_COUNTS, CYCLIC_PREV,
                         CYCLIC_NEXT, cyclic=True)
    return _once(("cyclic", half, levels), make)


def cyclic_rounds_case(half, levels, cap, count):
    def make():
        counts = (count, cap, 0)
        pts = _table(41, counts, cap, margin=(0, 26), seam=24)
        return TrackCase("cyclic rounds half %d levels %d count %d" % (half, levels, count), _pairs(True), levels, half, pts, counts,
                         (0, 4, 2), (1, 5, 3), cyclic=True, fb_max=FB_MAX)
    return _once(("cyclic rounds", half), make)


# ---- the tracker's reference ---------------------------------------------------------------------------------------------------------
def _pyramids(case):
    mod = reflk_cyclic if case.cyclic else reflk
    return _once(("pyr", id(case.gray), case.levels, case.cyclic), lambda: mod.pyramid_set(case.gray, case.levels))


def track_reference(case):
    """(next, status, err[, back]) as the stage must leave buffers that started as case.sentinels(); with `live`, the reference
    runs on those problems alone and every other problem keeps the sentinels."""
    def make():
        mod = reflk_cyclic if case.cyclic else reflk
        out = case.sentinels()
        rows = slice(None) if case.live is None else np.asarray(case.live)
        res = mod.track_problems(_pyramids(case), case.prev_img[rows], case.next_img[rows], case.pts[rows], case.n[rows], case.half,
                                 MAX_ITER, next_pts=None if case.guess is None else case.guess[rows], fb_max=case.fb_max,
                                 out=tuple(o[rows] for o in out))
        for o, r in zip(out, res):
            o[rows] = r
        return _frozen(*out[:len(res)])
    return _once(("track reference", case.key), make)


def forward_status(case):
    """The status of the same case without the forward-backward check (what the check may clear)."""
    def make():
        plain = TrackCase(case.key + " forward", case.gray, case.levels, case.half, case.pts, case.n, case.prev_img, case.next_img,
                          cyclic=case.cyclic, guess=case.guess, live=case.live)
        return track_reference(plain)[1]
    return _once(("forward status", case.key), make)


def later_round_rows(case):
    """(problem, row) of every point a later round of the keypoint loop tracks, among the problems that have an image."""
    ok = (case.prev_img >= 0) & (case.prev_img < len(case.gray)) & (case.next_img >= 0) & (case.next_img < len(case.gray))
    return [(p, k) for p in np.nonzero(ok)[0] for k in range(case.first_round, min(int(case.n[p]), case.cap))]


# ---- sosvo_refine_stereo_lk ------------------------------------------------------------------------------------------------------------
class StereoCase:
    def __init__(self, key, nmask, gray, kp_top, n_top, kp_bot, n_bot, keys, opts, min_disp=-1.0, max_hdiff=0.0):
        self.key, self.nmask, self.opts, self.min_disp, self.max_hdiff = key, nmask, opts, min_disp, max_hdiff
        self.gray, self.kp_top, self.kp_bot, self.keys = gray, kp_top, kp_bot, keys
        self.n_top, self.n_bot = np.asarray(n_top, np.int32), np.asarray(n_bot, np.int32)
        self.nprob, self.cap = kp_bot.shape[:2]
        _frozen(self.gray, self.kp_top, self.kp_bot, self.keys, self.n_top, self.n_bot)

    def __repr__(self):
        return self.key


STEREO_SHIFTS = (refstereolk.SHIFTS[0], refstereolk.SHIFTS[2])          # frame 0, frame 1


def _stereo_gray():
    return _once("stereo gray", lambda: _frozen(np.stack([reflk.texture(7, ROWS, COLS), reflk.texture(9, ROWS, COLS),
                                                          reflk.texture(7, ROWS, COLS, STEREO_SHIFTS[0]),
                                                          reflk.texture(9, ROWS, COLS, STEREO_SHIFTS[1])])))


STEREO_HALVES = (3, 5, 6, 9)
STEREO_N_BOT, STEREO_N_TOP = (16, 1, 0, 7, 16, 3), (16, 5, 3, 9, 12, 4)


def _stereo_tables(seed, nmask, cap, n_top, n_bot, jitter):
    """Top keypoints on and off the pixel grid, bottom keypoints = the true partner rounded, every third 1 px further (jitter:
    and up to a pixel off, so that no two rows of a problem are the same track); rows beyond the counts hold the sentinel."""
    rng = np.random.default_rng(seed)
    P = len(n_bot)
    kp_top = np.full((P, cap, 2), SENTINEL, np.float32)
    kp_bot = np.full((P, cap, 2), SENTINEL, np.float32)
    keys = np.full((P, cap), 0x12345678, np.uint32)          # (rows beyond n_bot: never read)
    for p in range(P):
        sh = np.asarray(STEREO_SHIFTS[p // nmask])
        for t in range(n_top[p]):
            xy = rng.uniform((24, 30), (COLS - 24, ROWS - 30))
            kp_top[p, t] = np.rint(xy) if t % 2 else xy
        for q in range(n_bot[p]):
            t = int(rng.integers(0, n_top[p]))
            kp_bot[p, q] = np.rint(kp_top[p, t].astype(np.float64) + sh) + ((1.0, -1.0) if q % 3 == 2 else (0.0, 0.0))
            if jitter:
                kp_bot[p, q] += rng.integers(-1, 2, 2)
            keys[p, q] = np.uint32(t | (int(rng.integers(0, 90)) << 20))
    return kp_top, kp_bot, keys


def stereo_case(half):
    """The scene of tests/test_gpu_stereo_lk.py: 2 frames, 3 masks, cap 16."""
    def make():
        tables = _once("stereo tables", lambda: _frozen(*_stereo_tables(41, 3, 16, STEREO_N_TOP, STEREO_N_BOT, False)))
        return StereoCase("stereo half %d" % half, 3, _stereo_gray(), tables[0], STEREO_N_TOP, tables[1], STEREO_N_BOT, tables[2],
                          dict(half=half, max_iter=MAX_ITER))
    return _once(("stereo", half), make)


GATHER_HALVES = (4, 6)
GATHER_CAP, GATHER_N_BOT, GATHER_N_TOP, GATHER_MAX_HDIFF = 600, (600, 257, 256, 0), (40, 40, 40, 5), 2.5


def gather_case(half):
    """2 frames, 2 masks, cap 600: the gather compacts problem 0 in three rounds of 256 rows.  About a third of the keys,
    scattered, are SOSVO_KEY_NONE, name a top row at or beyond n_top, or belong to a pair the pre-gate skips (|du| about 12 with
    max_hdiff 2.5 and max_shift 1.5); a few bottom keypoints are non-finite."""
    def make():
        def tables():
            rng = np.random.default_rng(59)
            kp_top, kp_bot, keys = _stereo_tables(43, 2, GATHER_CAP, GATHER_N_TOP, GATHER_N_BOT, True)
            for p, nb in enumerate(GATHER_N_BOT):
                u = rng.random(nb)
                for q in range(nb):
                    if u[q] < 0.12:
                        keys[p, q] = refstereolk.KEY_NONE
                    elif u[q] < 0.22:
                        keys[p, q] = np.uint32((GATHER_N_TOP[p] + int(rng.integers(0, 50))) | (7 << 20))
                    elif u[q] < 0.34:
                        kp_bot[p, q, 0] += np.float32(12.0)
                    elif u[q] < 0.36:
                        kp_bot[p, q, q & 1] = np.nan if q & 2 else np.inf
            return _frozen(kp_top, kp_bot, keys)
        t = _once("gather tables", tables)
        return StereoCase("gather half %d" % half, 2, _stereo_gray(), t[0], GATHER_N_TOP, t[1], GATHER_N_BOT, t[2],
                          dict(half=half, max_iter=MAX_ITER, max_shift=1.5), max_hdiff=GATHER_MAX_HDIFF)
    return _once(("gather", half), make)


def stereo_reference(case):
    """(kp_bot, status) after the stage; the status buffer started as 0xA5."""
    def make():
        return _frozen(*refstereolk.refine(case.gray, case.nmask, case.kp_top, case.n_top, case.kp_bot, case.n_bot, case.keys,
                                           min_disp=case.min_disp, max_hdiff=case.max_hdiff,
                                           status=np.full((case.nprob, case.cap), ST_SENTINEL, np.uint8),
                                           **dict(refstereolk.DEFAULTS, **case.opts)))
    return _once(("stereo reference", case.key), make)


def gathered(case, p):
    """Which of the rows q < n_bot[p] the gather hands to the tracker (the rule of refstereolk.refine up to the track)."""
    nb, nt = min(int(case.n_bot[p]), case.cap), min(int(case.n_top[p]), case.cap)
    s = refstereolk.bound(case.opts["half"], case.opts.get("max_shift"))
    keep = np.zeros(nb, bool)
    for q in range(nb):
        key = int(case.keys[p, q])
        t = key & refstereolk.KEY_IDX_MASK
        if key == refstereolk.KEY_NONE or t >= nt:
            continue
        (ut, vt), (ub, vb) = case.kp_top[p, t], case.kp_bot[p, q]
        keep[q] = bool(np.isfinite([ut, vt, ub, vb]).all()) and not refstereolk.pre_gate_skips(ut, vt, ub, vb, s, case.min_disp,
                                                                                              case.max_hdiff)
    return keep


# ---- sosvo_refine_subpix in the wide-grid form -------------------------------------------------------------------------------------------
SUBPIX_NIMG, SUBPIX_NMASK, SUBPIX_CAP, SUBPIX_ROWS, SUBPIX_COLS = 2, 2048, 80, 72, 96
SUBPIX_LIVE = ((0, 80), (5, 17), (1023, 1), (2047, 65), (2048, 17), (3333, 1), (4000, 1), (4095, 65))     # (problem, count)
SUBPIX_HALVES = (2, 5)
SUBPIX_FIRST_ROUND = 16


def _subpix_starts(rng, count):
    """count starts as in tests/test_gpu_subpix.py (integer ones near the rendered corners, fractional ones as ORB's level scales
    give, anywhere in the image); in every run of 16 rows an image corner, a NaN and a start outside the image."""
    kp = np.full((SUBPIX_CAP, 2), SENTINEL, np.float32)
    for k in range(count):
        cx, cy = 16 + 32 * rng.integers(0, 3), 18 + 36 * rng.integers(0, 2)
        if k % 16 == 3:
            kp[k] = (0, 0) if (k // 16) % 2 == 0 else (SUBPIX_COLS - 1, SUBPIX_ROWS - 1)
        elif k % 16 == 7:
            kp[k] = (np.nan, 20) if (k // 16) % 2 else (20, np.nan)
        elif k % 16 == 12:
            kp[k] = SUBPIX_COLS + 3.5, -2.25
        elif k % 4 == 0:
            kp[k] = cx + rng.integers(-2, 3), cy + rng.integers(-2, 3)
        elif k % 4 == 1:
            s = np.float32(1.2) ** rng.integers(1, 5)
            kp[k] = np.float32(np.rint((cx + rng.integers(-2, 3)) / s)) * s, np.float32(np.rint((cy + rng.integers(-2, 3)) / s)) * s
        elif k % 4 == 2:
            kp[k] = rng.uniform(-1, SUBPIX_COLS), rng.uniform(-1, SUBPIX_ROWS)
        else:
            kp[k] = rng.integers(0, SUBPIX_COLS), rng.integers(0, SUBPIX_ROWS)
    return kp


def subpix_wide_inputs():
    """-> (gray [2, 72, 96]: the six rendered corners of tests/test_gpu_subpix.py and noise, kp [4096, 80, 2], n [4096])."""
    def make():
        rng = np.random.default_rng(17)
        tiles = [refsubpix.render_corner(seed)[0][13:49, 15:47] for seed in range(6)]
        corners = np.vstack([np.hstack(tiles[:3]), np.hstack(tiles[3:])])
        gray = np.stack([corners, rng.integers(0, 256, (SUBPIX_ROWS, SUBPIX_COLS)).astype(np.uint8)])
        P = SUBPIX_NIMG * SUBPIX_NMASK
        kp = np.full((P, SUBPIX_CAP, 2), SENTINEL, np.float32)
        n = np.zeros(P, np.int32)
        for p, c in SUBPIX_LIVE:
            kp[p], n[p] = _subpix_starts(rng, c), c
        return _frozen(gray, kp, n)
    return _once("subpix wide", make)


def subpix_wide_reference(half):
    """kp after the stage: the reference refines the non-empty problems, each on its image; every other row is as it was."""
    def make():
        gray, kp, n = subpix_wide_inputs()
        out = kp.copy()
        for p, _ in SUBPIX_LIVE:
            image = p // SUBPIX_NMASK
            out[p] = refsubpix.refine_problems(gray[image:image + 1], 1, kp[p:p + 1], n[p:p + 1], half, MAX_ITER)[0]
        return _frozen(out)
    return _once(("subpix wide reference", half), make)
