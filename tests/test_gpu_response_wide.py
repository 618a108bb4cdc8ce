"""The corner-response kernel in its two-columns-per-lane form (the default from 8 columns on) and in its one-column form
(below that, or under SOSVO_HINT_ROLLING_NARROW), through sosvo_detect_gft_candidates, against oracle.min_eigen:

* per region (image, row chunk, strip) the records are exactly the positive 3x3 local maxima of the oracle's response that
  lie inside some mask, in the region's columns and rows and off the image's outermost rows and columns (the rule of
  goodFeaturesToTrack, which the one-column form has always applied), row-major and by ascending x, with the response's
  bits -- which fixes the set, the order and wcnt at once;
* the per-mask maxima equal the oracle's over all of a mask's pixels, in the order-preserving integer form;
* both forms give the same set per image, and detect_gft gives the same keypoints, counts and status in both forms,
  equal to the oracle's selection.

Shapes: one strip, a full wave of two strips, one column more, odd strip counts; heights from 3 rows to two chunks; 1, 12
and 32 masks with one and two images per mask set; bounding boxes that start and end on the columns 60 .. 62 and on the
chunk border; mask pixels in the first and last column, a band of rows without mask pixels, pixels in two masks, an empty
mask, a mask over a constant region (responses <= 0), a plateau of equal responses that makes every pixel of a region a
candidate, and exactly tied maxima in the two columns of one lane and across a lane border.  The oracle's response is
computed once per distinct image."""
import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

COLS = [3, 4, 5, 61, 62, 63, 122, 123, 124, 125, 183, 184, 245]
ROWS = [3, 4, 5, 26, 50]
TILE = np.array([[255, 0, 0, 0], [255, 0, 0, 0], [255, 255, 0, 255]], dtype=np.uint8)  # a plateau of equal responses


def _ordered(f):
    u = np.float32(f).view(np.uint32)
    return int(~u & 0xFFFFFFFF) if u & 0x80000000 else int(u | 0x80000000)


def _local_maxima(eig):
    """Boolean map of the positive 3x3 local maxima off the outermost rows and columns."""
    rows, cols = eig.shape
    out = np.zeros(eig.shape, bool)
    if rows < 3 or cols < 3:
        return out
    nb = np.full((rows - 2, cols - 2), -np.inf, np.float32)
    for dy in range(3):
        for dx in range(3):
            nb = np.maximum(nb, eig[dy:dy + rows - 2, dx:dx + cols - 2])
    c = eig[1:-1, 1:-1]
    out[1:-1, 1:-1] = (c == nb) & (c > 0)
    return out


def _masks(rng, rows, cols, nmask, nsets):
    """Sector masks that share their boundary column (a pixel in two masks), reach the first and the last column, leave a
    band of rows and a few columns without any mask, and -- with more than two masks -- leave the last mask empty."""
    bits = np.zeros((nsets, rows, cols), np.uint32)
    live = nmask - 1 if nmask > 2 else nmask
    for s in range(nsets):
        edges = np.linspace(0, cols - 1, live + 1).astype(int)
        for m in range(live):
            bits[s, :, edges[m]: edges[m + 1] + 1] |= np.uint32(1 << m)
        if rows >= 8:
            a = rows // 2 - 1 + s
            bits[s, a: a + 3] = 0                       # a band of rows without mask pixels
        if cols >= 20:
            x = int(rng.integers(4, cols - 8))
            bits[s, :, x: x + 3] = 0
        if rows >= 5:
            bits[s, 0, : cols // 2] = 0
    return bits


def _run_candidates(ctx, t_img, t_bits, ipm, nmask):
    r = ctx.detect_gft_candidates(t_img, t_bits, ipm, nmask)
    ctx.synchronize()
    r["cand"], r["wcnt"], r["mstat"] = r["cand"].cpu().numpy(), r["wcnt"].cpu().numpy(), r["mstat"].cpu().numpy()
    return r


def _check_form(r, imgs, eigs, bits, ipm, nmask, tag):
    """One form's records, counts and maxima against the oracle; returns the per-image record sets."""
    NI, rows, cols = imgs.shape
    w, strips, nchunks, cr, wcap = r["strip_w"], r["strips"], r["nchunks"], r["chunk_rows"], r["wcap"]
    assert strips == -(-cols // w) and nchunks * cr >= rows and r["regions"] == NI * strips * nchunks, tag
    assert wcap >= cr * w
    mask_all = np.uint32((1 << nmask) - 1 if nmask < 32 else 0xFFFFFFFF)
    sets = []
    for i in range(NI):
        mb = bits[i // ipm] & mask_all
        cmap = _local_maxima(eigs[i]) & (mb != 0)
        got_set = set()
        for c in range(nchunks):
            for s in range(strips):
                reg = (i * nchunks + c) * strips + s
                ys, xs = np.nonzero(cmap[c * cr: (c + 1) * cr, s * w: (s + 1) * w])   # row-major, ascending x
                ys, xs = ys + c * cr, xs + s * w
                want = np.stack([eigs[i][ys, xs].view(np.uint32), (ys.astype(np.uint32) << 16) | xs.astype(np.uint32)], axis=1)
                n = int(r["wcnt"][reg])
                assert n == len(want), "%s: image %d chunk %d strip %d: wcnt %d, oracle %d" % (tag, i, c, s, n, len(want))
                assert n <= wcap
                assert np.array_equal(r["cand"][reg, :n], want), "%s: image %d chunk %d strip %d: records differ" % (tag, i, c, s)
                got_set |= {tuple(v) for v in r["cand"][reg, :n].tolist()}
        sets.append(got_set)
        for m in range(nmask):
            inside = ((mb >> np.uint32(m)) & 1).astype(bool)
            want_max = _ordered(eigs[i][inside].max()) if inside.any() else 0
            assert int(r["mstat"][i * nmask + m, 0]) == want_max, "%s: image %d mask %d: maximum" % (tag, i, m)
    return sets


def _check_all(ctx, imgs, bits, ipm, nmask, tag, cap=64, max_corners=0, select=True):
    """Both forms through the candidates entry point and through detect_gft.  Returns the default form's result."""
    imgs, bits = np.ascontiguousarray(imgs), np.ascontiguousarray(bits)
    eigs = [oracle.min_eigen(im) for im in imgs]
    t_img, t_bits = torch.from_numpy(imgs.copy()).to(ctx.device), torch.from_numpy(bits.copy()).to(ctx.device)
    res, det = {}, {}
    try:
        for form in ("default", "narrow"):
            ctx.set_hint_rolling_narrow(form == "narrow")
            res[form] = _run_candidates(ctx, t_img, t_bits, ipm, nmask)
            if select:
                kp, n, status = ctx.detect_gft(t_img, t_bits, ipm, nmask, cap, max_corners=max_corners)
                ctx.synchronize()
                det[form] = (kp.cpu().numpy(), n.cpu().numpy(), status.cpu().numpy())
    finally:
        ctx.set_hint_rolling_narrow(False)
    cols = imgs.shape[2]
    assert res["narrow"]["strip_w"] == 58 and res["default"]["strip_w"] == (61 if cols >= 8 else 58), tag
    sets = {form: _check_form(res[form], imgs, eigs, bits, ipm, nmask, tag + " " + form) for form in res}
    assert sets["default"] == sets["narrow"], tag
    if select:
        (kp_d, n_d, st_d), (kp_n, n_n, st_n) = det["default"], det["narrow"]
        assert np.array_equal(n_d, n_n) and np.array_equal(st_d, st_n), tag
        for p in range(len(n_d)):
            i, m = divmod(p, nmask)
            want, _ = oracle.gft_select(eigs[i], bits[i // ipm], m, 0.01, 5.0, max_corners)
            want = want[:cap]
            assert n_d[p] == len(want), "%s: problem %d: %d keypoints, oracle %d" % (tag, p, n_d[p], len(want))
            assert np.array_equal(kp_d[p, : n_d[p]], want) and np.array_equal(kp_n[p, : n_n[p]], want), (tag, p)
        assert not st_d.any(), tag
    return res["default"], sets["default"]


@pytest.mark.parametrize("cols", COLS)
def test_response_forms_equal_the_oracle(ctx, cols):
    rng = np.random.default_rng(cols)
    k = COLS.index(cols)
    for j, rows in enumerate(ROWS):
        nmask = (1, 12, 32)[(k + j) % 3]
        ipm = 1 + (k + j) % 2
        imgs = rng.integers(0, 256, (2, rows, cols), dtype=np.uint8)
        pr, pc = min(rows, 20), min(cols // 2, 40)                                      # a plateau of equal responses in a corner
        imgs[1, :pr, :pc] = np.tile(TILE, (pr // 3 + 1, pc // 4 + 1))[:pr, :pc]
        bits = _masks(rng, rows, cols, nmask, 2 // ipm)
        _, sets = _check_all(ctx, imgs, bits, ipm, nmask, "rows %d cols %d nmask %d ipm %d" % (rows, cols, nmask, ipm))
        if rows >= 26 and cols >= 61:
            assert all(len(s) > 20 for s in sets)


def test_bounding_boxes_on_strip_and_chunk_borders(ctx):
    """Masks whose boxes start and end on the columns 60, 61 and 62 (the border of the first 61-column strip; 58 is the
    one-column form's) and on the rows 24 .. 26 (50 rows: two chunks of 25)."""
    rng = np.random.default_rng(6162)
    rows, cols = 50, 184
    imgs = rng.integers(0, 256, (2, rows, cols), dtype=np.uint8)
    boxes = [(0, 50, 60, 62), (0, 50, 61, 63), (0, 50, 62, 122), (0, 50, 0, 61), (0, 50, 0, 62), (25, 50, 122, 184),
             (0, 25, 122, 184), (24, 26, 57, 60), (26, 50, 58, 61), (0, 24, 183, 184), (25, 26, 0, 1), (10, 40, 61, 62)]
    bits = np.zeros((1, rows, cols), np.uint32)
    for m, (y0, y1, x0, x1) in enumerate(boxes):
        bits[0, y0:y1, x0:x1] |= np.uint32(1 << m)
    res, _ = _check_all(ctx, imgs, bits, 2, len(boxes), "boxes")
    assert res["nchunks"] == 2 and res["chunk_rows"] == 25 and res["strips"] == 4


def test_mask_over_a_constant_region(ctx):
    """Responses <= 0 under a whole mask: its maximum is the oracle's (0.0, not "no pixel"), it has no candidates and no
    keypoints, status 0 -- beside a mask with texture and an empty one."""
    rng = np.random.default_rng(9)
    rows, cols = 40, 130
    imgs = rng.integers(0, 256, (1, rows, cols), dtype=np.uint8)
    imgs[0, :, :70] = 93
    bits = np.zeros((1, rows, cols), np.uint32)
    bits[0, 4:36, 3:60] = 1
    bits[0, 2:38, 80:129] = 2
    res, sets = _check_all(ctx, imgs, bits, 1, 3, "constant")
    assert oracle.min_eigen(imgs[0])[4:36, 3:60].max() <= 0
    assert int(res["mstat"][0, 0]) == _ordered(0.0) and int(res["mstat"][2, 0]) == 0
    assert all(x >= 80 for (_, yx) in sets[0] for x in [yx & 0xFFFF]) and len(sets[0]) > 10


def test_plateau_makes_every_pixel_of_a_region_a_candidate(ctx):
    """An exactly periodic texture: equal positive responses everywhere, so a region away from the border holds a record for
    every one of its pixels (chunk_rows * strip width of them: what wcap is sized for)."""
    rows, cols = 120, 256
    imgs = np.tile(TILE, (rows // 3 + 1, cols // 4 + 1))[None, :rows, :cols].copy()
    bits = np.ones((1, rows, cols), np.uint32)
    res, _ = _check_all(ctx, imgs, bits, 1, 1, "plateau", select=False)
    cr, w, strips = res["chunk_rows"], res["strip_w"], res["strips"]
    assert res["nchunks"] >= 3 and strips >= 4
    reg = (0 * res["nchunks"] + 1) * strips + 1                    # second chunk, second strip: no border pixel
    assert int(res["wcnt"][reg]) == cr * w and cr * w <= res["wcap"] < cr * w + 64


@pytest.mark.parametrize("axis", [21, 22, 61, 62])
def test_exactly_tied_maxima_in_neighbouring_columns(ctx, axis):
    """A left-right symmetric image: the response is symmetric about the axis between the columns axis - 1 and axis, so a
    maximum in one of them is tied, bit for bit, with its mirror image in the other.  The lanes hold the column pairs
    (odd, even): axis 22 and 62 put the tie into the two columns of one lane (62: of the first lane of the second strip's
    half of the wave), axis 21 and 61 across a lane border (61: across the border of the two strips)."""
    rows = 30
    for seed in range(200):
        rng = np.random.default_rng(1000 * axis + seed)
        half = rng.integers(0, 256, (rows, axis), dtype=np.uint8)
        img = np.concatenate([half, half[:, ::-1]], axis=1)
        e = oracle.min_eigen(img)
        lm = _local_maxima(e)
        ys = np.nonzero(lm[:, axis - 1] & lm[:, axis])[0]
        if len(ys):
            break
    assert len(ys), "no symmetric image with a tied pair on the axis was found"
    y = int(ys[0])
    assert e[y, axis - 1] == e[y, axis] > 0
    cols = img.shape[1]
    bits = np.ones((1, rows, cols), np.uint32)
    res, sets = _check_all(ctx, img[None], bits, 1, 1, "tie at %d" % axis)
    v = int(e[y, axis].view(np.uint32))
    assert (v, (y << 16) | (axis - 1)) in sets[0] and (v, (y << 16) | axis) in sets[0]
