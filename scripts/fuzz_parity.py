#!/usr/bin/env python3
"""Differential fuzzing of the stage entry points against the CPU oracle (test infrastructure: the oracle is the checker).

    python scripts/fuzz_parity.py --minutes 10 --seed 1 [--stages median,gft,fast,agast,match,radius,orb,unwrap,ransac,describe,relpose,l2sort,pipeline,rgbd,batch,cross_check,gated_match]

Every case draws its own sizes and parameters (image sizes around the strip / chunk / tile borders of the kernels, omni
frames larger than 4 MB and at the 16384 limits for the unwrap table in about one `unwrap` case of eight, ragged
problem counts, empty masks, fractional minimum distances, budgets that end a selection inside a round, duplicate
descriptors, ...) from a generator seeded by (--seed, case number), runs the HIP stage through the C ABI and compares the
result with the oracle's bit for bit.  The first mismatch stops the run and prints the stage, the case number and the drawn
parameters: `--stages <stage> --first-case <n> --cases 1` with the same seed replays it.  Prints a progress line every ~20 s.
A case that only trips a documented capacity (status flags, a frame_cap cut) counts as `flagged`, not as a mismatch -- except
GFT's candidate limit (status bit 0 of sosvo_detect_gft), whose result is defined: such a case is compared like any other.  A
draw the entry point refuses, or a stage that ends short of --cases (or with no case at all) when time runs out, makes the
run end INCOMPLETE with exit status 2: only a run in which every stage completed its cases ends "all identical".
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle  # noqa: E402
from oracle import flow  # noqa: E402
import unwrap_cases  # noqa: E402  (tests/)
from vo_single_camera_sos_amd import orb_pattern  # noqa: E402
from vo_single_camera_sos_amd.device import Context, SosvoError  # noqa: E402


def _dev(ctx, *arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device) for a in arrs]


def _image(rng, rows, cols, kind):
    """gray test images: noise, smooth texture, blobs on black, constant"""
    if kind == 0:
        return rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    if kind == 1:
        a = rng.normal(0, 1, (rows // 4 + 2, cols // 4 + 2))
        a = np.kron(a, np.ones((4, 4)))[:rows, :cols]
        return np.clip(128 + 60 * a + rng.normal(0, 6, (rows, cols)), 0, 255).astype(np.uint8)
    if kind == 2:
        img = np.zeros((rows, cols), np.uint8)
        for _ in range(int(rng.integers(1, 60))):
            y, x, s = int(rng.integers(0, rows)), int(rng.integers(0, cols)), int(rng.integers(1, 7))
            img[y:y + s, x:x + s] = rng.integers(30, 256)
        return img
    return np.full((rows, cols), int(rng.integers(0, 256)), np.uint8)


def _masks(rng, rows, cols, nmask):
    bits = np.zeros((rows, cols), np.uint32)
    kind = int(rng.integers(0, 4))
    if kind == 0:     # azimuthal sectors sharing their border columns, a few rows out
        edges = np.linspace(0, cols - 1, nmask + 1).astype(int)
        for m in range(nmask):
            bits[:, edges[m]:edges[m + 1] + 1] |= np.uint32(1 << m)
        bits[:int(rng.integers(0, 4))] = 0
    elif kind == 1:   # random rectangles (overlapping, possibly empty)
        for m in range(nmask):
            y0, y1 = sorted(rng.integers(0, rows, 2))
            x0, x1 = sorted(rng.integers(0, cols, 2))
            bits[y0:y1, x0:x1] |= np.uint32(1 << m)
    elif kind == 2:   # everything in every mask
        bits[:] = np.uint32((1 << nmask) - 1)
    else:             # random pixels
        for m in range(nmask):
            bits |= (rng.random((rows, cols)) < rng.random()).astype(np.uint32) << np.uint32(m)
    return bits


def fuzz_median(ctx, rng):
    k = int(rng.choice([3, 5, 11]))
    rows, cols, n = int(rng.integers(1, 90)), int(rng.integers(1, 260)), int(rng.integers(1, 4))
    if rng.random() < 0.08:
        rows, cols = int(rng.integers(90, 300)), int(rng.integers(260, 1500))
    img = rng.integers(0, 256, (n, rows, cols, 3), dtype=np.uint8)
    if rng.random() < 0.3:
        img[:, :, :, :] = (img >> int(rng.integers(4, 8))) << 4   # few distinct values: many ties inside a window
    params = dict(ksize=k, rows=rows, cols=cols, nimg=n)
    (t,) = _dev(ctx, img)
    got = ctx.median_gray(t, k)
    ctx.synchronize()
    got = got.cpu().numpy()
    for i in range(n):
        if not np.array_equal(got[i], oracle.median_gray(img[i], k)):
            return params, "image %d differs" % i
    return params, None


def fuzz_gft(ctx, rng):
    rows, cols = int(rng.integers(3, 140)), int(rng.integers(3, 420))
    nmask, ni = int(rng.integers(1, 7)), int(rng.integers(1, 4))
    cap = int(rng.choice([16, 64, 512, 1024, 2048]))
    shape_mode = rng.random()
    if shape_mode < 0.08:      # more than 1024 problems in one launch: the four-wave selection / descriptor workgroups
        rows, cols, nmask, ni, cap = int(rng.integers(8, 36)), int(rng.integers(20, 90)), int(rng.integers(20, 33)), int(rng.integers(36, 60)), 64
    elif shape_mode < 0.16:    # a large image: many strips and row chunks
        rows, cols = int(rng.integers(140, 320)), int(rng.integers(420, 1500))
    q = float(10 ** rng.uniform(-3, -0.3))
    md = float(rng.choice([0.0, 0.7, 1.0, 1.5, 2.0, 3.0, 5.0, 7.5, 12.0, 25.0, 33.3, 40.0, 60.0]))
    mc = int(rng.choice([0, 1, 7, 50, 300, 1000]))
    params = dict(rows=rows, cols=cols, nmask=nmask, nimg=ni, cap=cap, quality=q, min_distance=md, max_corners=mc)
    kinds = rng.integers(0, 4, ni)
    imgs = np.stack([_image(rng, rows, cols, int(k)) for k in kinds])
    bits = _masks(rng, rows, cols, nmask)[None]
    t_img, t_bits = _dev(ctx, imgs, bits)
    kp, n, status = ctx.detect_gft(t_img, t_bits, ni, nmask, cap, quality=q, min_distance=md, max_corners=mc)
    ctx.synchronize()
    kp, n, status = kp.cpu().numpy(), n.cpu().numpy(), status.cpu().numpy()
    flagged = False
    for i in range(ni):
        eig = oracle.min_eigen(imgs[i])
        for m in range(nmask):
            # (more candidates than the selection sorts -- status bit 0 -- is a defined result: the CAND strongest are kept)
            cand_cap = oracle.gft_cand_cap(cap)
            want, _, count = oracle.gft_select(eig, bits[0], m, q, md, mc, cand_cap=cand_cap, with_count=True)
            p = i * nmask + m
            if status[p] & 2:     # the mask's cell grid does not fit on chip: at most 1024 corners (sosvo.h)
                flagged = True
                continue
            if status[p] != (1 if count > cand_cap else 0):
                return params, "image %d mask %d: status %d with %d candidates" % (i, m, status[p], count)
            want = want[:cap]
            if n[p] != len(want) or not np.array_equal(kp[p, :n[p]], want):
                return params, "image %d mask %d: %d corners, oracle %d" % (i, m, n[p], len(want))
    return params, ("flagged" if flagged else None)


def _fast_like(ctx, rng, agast):
    import refflow
    rows, cols = int(rng.integers(8, 120)), int(rng.integers(8, 330))
    if rng.random() < 0.08:
        rows, cols = int(rng.integers(120, 400)), int(rng.integers(330, 1500))
    nmask, ni = int(rng.integers(1, 5)), int(rng.integers(1, 4))
    cap = int(rng.choice([8, 64, 1024, 4096]))
    thr = int(rng.choice([1, 5, 10, 20, 40, 80]))
    params = dict(rows=rows, cols=cols, nmask=nmask, nimg=ni, cap=cap, threshold=thr)
    imgs = np.stack([_image(rng, rows, cols, int(rng.integers(0, 4))) for _ in range(ni)])
    bits = _masks(rng, rows, cols, nmask)[None]
    t_img, t_bits = _dev(ctx, imgs, bits)
    fn = ctx.detect_agast if agast else ctx.detect_fast
    kp, n, status = fn(t_img, t_bits, ni, nmask, cap, threshold=thr)
    ctx.synchronize()
    kp, n, status = kp.cpu().numpy(), n.cpu().numpy(), status.cpu().numpy()
    ref = refflow.agast_keypoints if agast else refflow.fast_keypoints
    for i in range(ni):
        for m in range(nmask):
            want = ref(imgs[i], bits[0], m, thr)
            p = i * nmask + m
            if agast and status[p] & 2:
                continue
            if n[p] != min(len(want), cap) or not np.array_equal(kp[p, :n[p]], want[:cap]):
                return params, "image %d mask %d: %d corners, oracle %d" % (i, m, n[p], len(want))
    return params, None


def fuzz_fast(ctx, rng):
    return _fast_like(ctx, rng, False)


def fuzz_agast(ctx, rng):
    return _fast_like(ctx, rng, True)


def _descriptors(rng, P, Sq, St, nq, nt):
    q = rng.integers(0, 256, (P, Sq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (P, St, 32), dtype=np.uint8)
    mode = int(rng.integers(0, 4))
    for p in range(P):
        if mode == 1 and nq[p] and nt[p]:      # noisy copies + exact duplicates: ties
            m = max(1, min(nq[p], nt[p]) // 2)
            src, dst = rng.integers(0, nq[p], m), rng.integers(0, nt[p], m)
            t[p, dst] = q[p, src] ^ np.packbits(rng.random((m, 32, 8)) < 0.04, axis=-1)[..., 0]
            t[p, dst[:m // 3]] = q[p, src[:m // 3]]
        elif mode == 2:                        # extremes: all zeros / all ones rows
            t[p, ::3] = 0
            q[p, ::5] = 255
        elif mode == 3 and nt[p]:              # every train row the same
            t[p, :] = t[p, 0]
    return q, t


def fuzz_match(ctx, rng):
    P = int(rng.integers(1, 20))
    Sq, St = int(rng.choice([1, 17, 64, 130, 256, 300, 1024, 2100])), int(rng.choice([1, 33, 128, 129, 255, 700, 2100]))
    if P * Sq * St > 3e7:
        P = max(1, int(3e7 // (Sq * St)))
    k = int(rng.integers(1, 3))
    nq = rng.integers(0, Sq + 1, P).astype(np.int32)
    nt = rng.integers(0, St + 1, P).astype(np.int32)
    if rng.random() < 0.5:
        nq[:], nt[:] = Sq, St
    params = dict(P=P, q_stride=Sq, t_stride=St, k=k, nq=nq.tolist()[:8], nt=nt.tolist()[:8])
    q, t = _descriptors(rng, P, Sq, St, nq, nt)
    tq, tt, tnq, tnt = _dev(ctx, q, t, nq, nt)
    keys = ctx.match_hamming(tq, tt, tnq, tnt, k=k)
    ctx.synchronize()
    keys = keys.cpu().numpy()
    for p in range(P):
        want = oracle.match_hamming(q[p, :nq[p]], t[p, :nt[p]], k=k)
        if not np.array_equal(keys[p, :nq[p]], want):
            return params, "problem %d" % p
    return params, None


def fuzz_cross_check(ctx, rng):
    """The mutual-consistency filter (sosvo_cross_check_matches on the keys of two sosvo_match_hamming calls, then the sort)
    against the definition (tests/refmatch.py): query i keeps its best train j iff the best query of j is i.  Sizes 0 and 1, the
    32-query / 128-train tile edges of the matcher, and half of the cases through slot tables over one descriptor store."""
    from refmatch import NONE, Matching
    sizes = [0, 1, 2, 31, 32, 33, 127, 128, 129, 255, 257, 300]
    slots = rng.random() < 0.5
    if slots:            # a store of blocks, problems = (query block, train block) pairs, a block may meet itself
        nb, S = int(rng.integers(1, 6)), int(rng.choice([1, 33, 130, 320]))
        cnt = np.minimum(rng.choice(sizes, nb), S).astype(np.int32)
        store, _ = _descriptors(rng, nb, S, S, cnt, cnt)
        for b in range(1, nb):   # later blocks re-observe earlier ones: several queries per train
            m = min(cnt[b], cnt[b - 1])
            if m:
                store[b, :m:2] = store[b - 1, rng.integers(0, max(1, m // 2), len(range(0, m, 2)))]
        P = int(rng.integers(1, 9))
        qs, ts = rng.integers(0, nb, P).astype(np.int32), rng.integers(0, nb, P).astype(np.int32)
        q = t = store
        nq = nt = cnt
        Sq = St = S
    else:
        P = int(rng.integers(1, 9))
        Sq, St = int(rng.choice([1, 33, 130, 320])), int(rng.choice([1, 33, 129, 320]))
        nq = np.minimum(rng.choice(sizes, P), Sq).astype(np.int32)
        nt = np.minimum(rng.choice(sizes, P), St).astype(np.int32)
        q, t = _descriptors(rng, P, Sq, St, nq, nt)
        qs = ts = np.arange(P, dtype=np.int32)
    alias = bool(rng.integers(0, 2))
    params = dict(P=P, slots=slots, q_stride=Sq, t_stride=St, nq=nq.tolist(), nt=nt.tolist(), q_slot=qs.tolist(), t_slot=ts.tolist(),
                  alias=alias)
    tq, tt, tnq, tnt, tqs, tts = _dev(ctx, q, t, nq, nt, qs, ts)
    fwd_slots = dict(q_slot=tqs, t_slot=tts) if slots else {}
    rev_slots = dict(q_slot=tts, t_slot=tqs) if slots else {}
    fwd = ctx.match_hamming(tq, tt, tnq, tnt, k=1, **fwd_slots)
    rev = ctx.match_hamming(tt, tq, tnt, tnq, k=1, **rev_slots)
    out, n_kept = ctx.cross_check_matches(fwd, rev, tnq, tnt, keys_out=fwd if alias else None, **fwd_slots)
    order = ctx.sort_matches(out, tnq, q_slot=tqs if slots else None)
    ctx.synchronize()
    out, n_kept, order = out.cpu().numpy()[:, :, 0], n_kept.cpu().numpy(), order.cpu().numpy()
    for p in range(P):
        n, m = int(nq[qs[p]]), int(nt[ts[p]])
        want = Matching(mutual=True).kept(q[qs[p], :n], t[ts[p], :m], None, None, None)
        if not np.array_equal(out[p, :n], want):
            return params, "problem %d: keys" % p
        if n_kept[p] != int((want != NONE).sum()):
            return params, "problem %d: n_kept" % p
        if not np.array_equal(order[p, :n], oracle.sort_matches(want)):
            return params, "problem %d: order" % p
    return params, None


def fuzz_gated_match(ctx, rng):
    """sosvo_match_hamming_gated against its definition in numpy (tests/refmatch.py): key(i) = min over the trains j that pass
    oracle.pixel_gates (on the float32 positions converted to double) of (hamming << 20 | j), SOSVO_KEY_NONE without one or
    when the winner's distance exceeds the cap; then the sort.  Random sizes around the 32-query / 128-train tile edges, gates
    with either side disabled, limits that sit exactly on a position difference, caps 0 .. 256, half of the cases through
    slot tables over one store, a random share of the problems reversed (the role-swapped problems of a cross-checked
    step).  With both sides disabled and no cap the keys must also be those of sosvo_match_hamming."""
    from refmatch import Matching
    sizes = [0, 1, 2, 31, 32, 33, 127, 128, 129, 255, 257, 300]
    slots = rng.random() < 0.5
    if slots:
        nb, S = int(rng.integers(1, 6)), int(rng.choice([1, 33, 130, 320]))
        cnt = np.minimum(rng.choice(sizes, nb), S).astype(np.int32)
        store, _ = _descriptors(rng, nb, S, S, cnt, cnt)
        for b in range(1, nb):
            m = min(cnt[b], cnt[b - 1])
            if m:
                store[b, :m:2] = store[b - 1, rng.integers(0, max(1, m // 2), len(range(0, m, 2)))]
        P = int(rng.integers(1, 9))
        qs, ts = rng.integers(0, nb, P).astype(np.int32), rng.integers(0, nb, P).astype(np.int32)
        q = t = store
        nq = nt = cnt
        Sq = St = S
    else:
        P = int(rng.integers(1, 9))
        Sq, St = int(rng.choice([1, 33, 130, 320, 1024])), int(rng.choice([1, 33, 129, 320]))
        nq = np.minimum(rng.choice(sizes, P), Sq).astype(np.int32)
        nt = np.minimum(rng.choice(sizes, P), St).astype(np.int32)
        q, t = _descriptors(rng, P, Sq, St, nq, nt)
        qs = ts = np.arange(P, dtype=np.int32)
    # positions on a quarter-pixel grid inside a small window: many pairs sit exactly on a limit drawn from the same grid
    span = float(rng.choice([4.0, 16.0, 64.0]))
    grid = lambda shape: (np.round(rng.uniform(0.0, span, shape) * 4.0) / 4.0).astype(np.float32)  # noqa: E731
    qp = grid(q.shape[:2] + (2,))
    tp = qp if slots else grid(t.shape[:2] + (2,))
    if rng.random() < 0.3:                   # off-grid positions: differences that are not representable in float32
        qp = (qp + rng.uniform(0.0, 1e-3, qp.shape)).astype(np.float32)
        tp = qp if slots else (tp + rng.uniform(0.0, 1e-3, tp.shape)).astype(np.float32)
    min_dv = float(rng.choice([-1.0, 0.0, 0.25, 1.0, 3.5]))
    max_du = float(rng.choice([-1.0, 0.0, 0.25, 2.5, 7.75, 1e9]))
    cap = [None, 0, 1, 40, 64, 100, 128, 256][int(rng.integers(0, 8))]
    n_forward = int(rng.integers(0, P + 1))
    params = dict(P=P, slots=slots, q_stride=Sq, t_stride=St, nq=nq.tolist(), nt=nt.tolist(), q_slot=qs.tolist(), t_slot=ts.tolist(),
                  span=span, min_dv=min_dv, max_du=max_du, cap=cap, n_forward=n_forward)
    tq, tt, tqp, ttp, tnq, tnt, tqs, tts = _dev(ctx, q, t, qp, tp, nq, nt, qs, ts)
    sl = dict(q_slot=tqs, t_slot=tts) if slots else {}
    keys = ctx.match_hamming_gated(tq, tt, tqp, ttp, tnq, tnt, min_dv, max_du, cap, n_forward=n_forward, **sl)
    order = ctx.sort_matches(keys, tnq, q_slot=tqs if slots else None)
    plain = ctx.match_hamming(tq, tt, tnq, tnt, k=1, **sl) if (min_dv < 0 and max_du <= 0 and cap in (None, 256)) else None
    ctx.synchronize()
    keys, order = keys.cpu().numpy()[:, :, 0], order.cpu().numpy()
    for p in range(P):
        n, m = int(nq[qs[p]]), int(nt[ts[p]])
        want = Matching(gated=True, cap=cap).keys(q[qs[p], :n], t[ts[p], :m], qp[qs[p], :n], tp[ts[p], :m], (min_dv, max_du),
                                                  reverse=p >= n_forward)
        if not np.array_equal(keys[p, :n], want):
            return params, "problem %d: keys" % p
        if not np.array_equal(order[p, :n], oracle.sort_matches(want)):
            return params, "problem %d: order" % p
        if plain is not None and not np.array_equal(plain.cpu().numpy()[p, :n, 0], want):
            return params, "problem %d: differs from sosvo_match_hamming" % p
    return params, None


def fuzz_radius(ctx, rng):
    P = int(rng.integers(1, 8))
    Sq, St = int(rng.choice([1, 40, 200, 333])), int(rng.choice([1, 64, 257, 500]))
    nq = rng.integers(0, Sq + 1, P).astype(np.int32)
    nt = rng.integers(0, St + 1, P).astype(np.int32)
    maxd, cap = float(rng.choice([0, 20, 90, 110, 128, 300])), int(rng.choice([1, 4, 16]))
    params = dict(P=P, q_stride=Sq, t_stride=St, max_distance=maxd, cap=cap)
    q, t = _descriptors(rng, P, Sq, St, nq, nt)
    tq, tt, tnq, tnt = _dev(ctx, q, t, nq, nt)
    keys, cnt = ctx.match_radius(tq, tt, tnq, tnt, maxd, cap)
    ctx.synchronize()
    keys, cnt = keys.cpu().numpy(), cnt.cpu().numpy()
    for p in range(P):
        wk, wc = oracle.match_radius(q[p, :nq[p]], t[p, :nt[p]], maxd, cap)
        if not np.array_equal(cnt[p, :nq[p]], wc):
            return params, "problem %d: counts" % p
        for i in range(nq[p]):
            m = min(int(wc[i]), cap)
            if not np.array_equal(keys[p, i, :m], wk[i, :m]):
                return params, "problem %d query %d" % (p, i)
    return params, None


def fuzz_orb(ctx, rng):
    rows, cols = int(rng.integers(70, 150)), int(rng.integers(70, 400))
    if rng.random() < 0.08:
        rows, cols = int(rng.integers(150, 300)), int(rng.integers(400, 1500))
    nmask, ni = int(rng.integers(1, 4)), int(rng.integers(1, 3))
    nfeat, cap = int(rng.choice([10, 60, 230, 500])), int(rng.choice([64, 512, 1024]))
    params = dict(rows=rows, cols=cols, nmask=nmask, nimg=ni, nfeatures=nfeat, cap=cap)
    imgs = np.stack([_image(rng, rows, cols, int(rng.integers(0, 3))) for _ in range(ni)])
    bits = _masks(rng, rows, cols, nmask)[None]
    t_img, t_bits = _dev(ctx, imgs, bits)
    pyr = ctx.orb_mask_pyramid(t_bits, nmask)
    kp4, resp, n = ctx.detect_orb(t_img, pyr, ni, nmask, nfeat, cap)
    ctx.synchronize()
    kp_d, resp_d, n_d = kp4.cpu().numpy(), resp.cpu().numpy(), n.cpu().numpy()   # (describe_orb_levels compacts kp4 / n in place)
    (pattern,) = _dev(ctx, orb_pattern.orb_pattern())
    desc, _ = ctx.describe_orb_levels(t_img, kp4, n, nmask, pattern)
    ctx.synchronize()
    n2, desc = n.cpu().numpy(), desc.cpu().numpy()
    for i in range(ni):
        want = oracle.orb_detect(imgs[i], bits[0], nmask, nfeat, cap)
        for m in range(nmask):
            p = i * nmask + m
            wkp, wresp = want[m]
            if n_d[p] != len(wkp) or not np.array_equal(kp_d[p, :n_d[p]], wkp) or not np.array_equal(resp_d[p, :n_d[p]], wresp):
                k = min(n_d[p], len(wkp))
                bad = np.nonzero((kp_d[p, :k] != wkp[:k]).any(axis=1) | (resp_d[p, :k] != wresp[:k]))[0]
                first = int(bad[0]) if len(bad) else k
                return params, "image %d mask %d: keypoints (%d, oracle %d); first difference at %d of %d differing: got %s %r, oracle %s %r" % (
                    i, m, n_d[p], len(wkp), first, len(bad), kp_d[p, first].tolist() if first < n_d[p] else None,
                    float(resp_d[p, first]) if first < n_d[p] else None, wkp[first].tolist() if first < len(wkp) else None,
                    float(wresp[first]) if first < len(wkp) else None)
            wd, kept = oracle.orb_describe_levels(imgs[i], wkp)
            if n2[p] != len(kept) or not np.array_equal(desc[p, :n2[p]], wd):
                return params, "image %d mask %d: descriptors (%d, oracle %d)" % (i, m, n2[p], len(kept))
    return params, None


def fuzz_describe(ctx, rng):
    rows, cols = int(rng.integers(64, 200)), int(rng.integers(64, 500))
    nmask, ni = int(rng.integers(1, 5)), int(rng.integers(1, 4))
    cap = int(rng.choice([8, 128, 1024, 2048]))
    if rng.random() < 0.08:
        rows, cols, nmask, ni, cap = 64, int(rng.integers(64, 90)), int(rng.integers(20, 33)), int(rng.integers(36, 56)), 16
    angle = float(rng.choice([orb_pattern.GFT_KEYPOINT_ANGLE, 0.0, 37.5, 90.0, 180.0, 271.3]))
    params = dict(rows=rows, cols=cols, nmask=nmask, nimg=ni, cap=cap, angle=angle)
    imgs = np.stack([_image(rng, rows, cols, int(rng.integers(0, 3))) for _ in range(ni)])
    P = ni * nmask
    kp = np.zeros((P, cap, 2), np.float32)
    n = rng.integers(0, cap + 1, P).astype(np.int32)
    for p in range(P):
        whole = rng.random() < 0.7
        x, y = rng.uniform(0, cols, n[p]), rng.uniform(0, rows, n[p])
        kp[p, :n[p], 0], kp[p, :n[p], 1] = (x.round(), y.round()) if whole else (x, y)
        if n[p] >= 4:      # the border rule's edges
            kp[p, :4] = [[31.0, 31.0], [30.99, 40.0], [cols - 31.0, 40.0], [cols - 31.01, rows - 31.01]]
    pat = orb_pattern.orb_pattern()
    ca, sa = orb_pattern.angle_cos_sin(angle)
    t_img, t_kp, t_n, t_pat = _dev(ctx, imgs, kp, n, pat)
    desc = ctx.describe_orb(t_img, t_kp, t_n, nmask, t_pat, ca, sa)
    ctx.synchronize()
    desc, kp_out, n_out = desc.cpu().numpy(), t_kp.cpu().numpy(), t_n.cpu().numpy()
    blurred = [oracle.gauss7(im) for im in imgs]
    for p in range(P):
        wd, kept = oracle.orb_describe(blurred[p // nmask], kp[p, :n[p]], ca, sa, pat)
        if n_out[p] != len(kept) or not np.array_equal(kp_out[p, :len(kept)], kp[p, kept]):
            return params, "problem %d: border rule (%d kept, oracle %d)" % (p, n_out[p], len(kept))
        if not np.array_equal(desc[p, :len(kept)], wd):
            return params, "problem %d: descriptor bits" % p
    return params, None


def draw_unwrap(rng):
    """The frame, panorama and maps of an `unwrap` case (no GPU).  About one case in eight takes one of the frames larger
    than 4 MB of tests/unwrap_cases.py with its maps (a) - (d): taps beyond byte 2^22 of a frame, which the table stores in
    its edge format, W / H at the 16384 limit.  The others are small frames, never one the table form refuses (a frame
    holds 8 bytes after the start of its second row, 3 W (H - 1) >= 8: include/sosvo.h)."""
    large = rng.random() < 0.125
    if large:
        H, W = list(unwrap_cases.LARGE_FRAMES)[int(rng.integers(0, len(unwrap_cases.LARGE_FRAMES)))]
        rows, cols = int(rng.integers(5, 50)), int(rng.integers(16, 150))
    else:
        H, W = int(rng.integers(2, 80)), int(rng.integers(2, 120))
        if 3 * W * (H - 1) < 8:      # (2, 2), the one refused size of this range
            H += 1
        rows, cols = int(rng.integers(1, 50)), int(rng.integers(1, 150))
    nf, ksize = int(rng.integers(1, 4)), int(rng.choice([0, 3, 5, 11]))
    params = dict(H=H, W=W, rows=rows, cols=cols, nframes=nf, ksize=ksize, large=large)
    if large:
        mx, my = unwrap_cases.large_frame_maps(rng, H, W, (rows, cols))
        return params, mx, my
    span = float(rng.choice([1.0, 1.3, 4.0]))   # maps that stay inside / leave the frame
    mx = (rng.uniform(-0.5 * (span - 1) * W - 5, W * (1 + 0.5 * (span - 1)) + 5, (2, rows, cols))).astype(np.float32)
    my = (rng.uniform(-0.5 * (span - 1) * H - 5, H * (1 + 0.5 * (span - 1)) + 5, (2, rows, cols))).astype(np.float32)
    if rng.random() < 0.5:
        mx = np.round(mx * 64) / 64     # exact 1/64 fractions: the round-half-even cases of the 1/32-pixel grid
        my = np.round(my * 64) / 64
    mx[rng.random(mx.shape) < 0.02] = np.nan
    my[rng.random(my.shape) < 0.02] = np.inf
    return params, mx, my


def fuzz_unwrap(ctx, rng):
    params, mx, my = draw_unwrap(rng)
    H, W, nf, ksize = params["H"], params["W"], params["nframes"], params["ksize"]
    omni = rng.integers(0, 256, (nf, H, W, 3), dtype=np.uint8)
    masks = ((rng.random((2, H, W)) < rng.uniform(0.3, 1.0)).astype(np.uint8)) * 255
    use_mask = rng.random() < 0.7
    t_omni, t_masks, t_mx, t_my = _dev(ctx, omni, masks, mx.astype(np.float32), my.astype(np.float32))
    tm = t_masks if use_mask else None
    pano = ctx.unwrap(t_omni, tm, t_mx, t_my)
    table = ctx.unwrap_prepare(tm, t_mx, t_my, (H, W))
    pano_t = ctx.unwrap_table(t_omni, table)
    gray = ctx.unwrap_median_gray(t_omni, table, ksize)
    ctx.synchronize()
    pano, pano_t, gray = pano.cpu().numpy(), pano_t.cpu().numpy(), gray.cpu().numpy()
    for v in range(2):
        for f in range(nf):
            want = oracle.unwrap(omni[f], masks[v] if use_mask else None, mx[v], my[v])
            if not np.array_equal(pano[v, f], want):
                return params, "view %d frame %d: map form" % (v, f)
            if not np.array_equal(pano_t[v, f], want):
                return params, "view %d frame %d: table form" % (v, f)
            if not np.array_equal(gray[v * nf + f], oracle.median_gray(want, ksize)):
                return params, "view %d frame %d: fused unwrap + median + gray" % (v, f)
    return params, None


def fuzz_ransac(ctx, rng):
    import synth
    P = int(rng.integers(1, 6))
    S = int(rng.choice([8, 40, 130, 700]))
    noncentral = bool(rng.integers(0, 2))
    solver = str(rng.choice(["P3P", "GP3P", "EPNP", "TWOPT"] if True else []))
    if solver == "GP3P":
        noncentral = True
    if solver in ("EPNP", "TWOPT"):
        noncentral = False
    max_iter = int(rng.choice([1, 17, 64, 300]))
    adaptive = bool(rng.integers(0, 2))
    thr = float(rng.choice([synth.THR_5DEG, 1.0 - np.cos(np.deg2rad(0.5)), 1e-9]))
    seed = int(rng.integers(0, 2 ** 31))
    params = dict(P=P, S=S, noncentral=noncentral, solver=solver, max_iter=max_iter, adaptive=adaptive, thr=thr, seed=seed)
    problems = []
    for b in range(P):
        n = int(rng.integers(0, S + 1)) if rng.random() < 0.7 else S
        pr = synth.make_abs_pose_problem(rng, max(n, 1), inlier_frac=float(rng.choice([0.0, 0.2, 0.6, 1.0])),
                                         noise_deg=float(rng.choice([0.0, 0.2, 2.0])), noncentral=noncentral)
        if n == 0:
            pr = dict(pr, f=pr["f"][:0], p=pr["p"][:0], cam=None if pr["cam"] is None else pr["cam"][:0])
        if solver == "TWOPT":     # the identity-rotation solver: bearings of a pure translation
            pr["f"] = pr["f"]
        problems.append(pr)
    f = np.zeros((P, S, 3)); pp = np.zeros((P, S, 3)); cam = np.zeros((P, S), np.int32); n_arr = np.zeros(P, np.int32)
    for b, pr in enumerate(problems):
        k = pr["f"].shape[0]
        n_arr[b] = k
        f[b, :k], pp[b, :k] = pr["f"], pr["p"]
        if noncentral:
            cam[b, :k] = pr["cam"]
    tf, tp, tcam, tn = _dev(ctx, f, pp, cam, n_arr)
    kw = {}
    if noncentral:
        off, rot = _dev(ctx, problems[0]["cam_off"], problems[0]["cam_rot"])
        kw = dict(cam=tcam, cam_off=off, cam_rot=rot, cam_rot_identity=bool(rng.integers(0, 2)))
    flags = dict(epnp=solver == "EPNP", gp3p=solver == "GP3P", twopt=solver == "TWOPT")
    out = ctx.ransac_abs_pose(tf, tp, tn, thr, max_iter, seed=seed, adaptive=adaptive, want_counts=True, **flags, **kw)
    T0 = out["T"].clone()
    kw2 = {k: v for k, v in kw.items() if k != "cam_rot_identity"}
    Tr, cost, iters = ctx.refine_abs_pose(tf, tp, tn, out["T"].clone(), idx=out["idx"], m=out["n_inliers"], **kw2)
    ctx.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    T0, Tr, cost, iters = T0.cpu().numpy(), Tr.cpu().numpy(), cost.cpu().numpy(), iters.cpu().numpy()
    for b, pr in enumerate(problems):
        okw = dict(cam=pr["cam"], cam_off=pr["cam_off"], cam_rot=pr["cam_rot"]) if noncentral else {}
        want = oracle.ransac_abs_pose(pr["f"], pr["p"], thr, max_iter, seed=seed + b, adaptive=adaptive, want_counts=True, **flags, **okw)
        k, used = n_arr[b], want["iters_used"]
        if got["info"][b, 1] != used or got["info"][b, 0] != want["best_iter"] or got["info"][b, 2] != want["status"]:
            return params, "problem %d: iterations / winner / status (%s, oracle %d %d %d)" % (b, got["info"][b, :3].tolist(), want["best_iter"], used, want["status"])
        if not np.array_equal(got["counts"][b, :used], want["counts"][:used]):
            return params, "problem %d: hypothesis counts" % b
        if got["n_inliers"][b] != want["n_inliers"] or not np.array_equal(got["mask"][b, :k].astype(bool), want["mask"]):
            return params, "problem %d: inlier mask" % b
        if not np.array_equal(got["T"][b], want["T"]):
            return params, "problem %d: pose bits" % b
        if want["status"] == 0 and want["n_inliers"] >= 3:
            idx = np.nonzero(want["mask"])[0].astype(np.int32)
            wT, wcost, wit = oracle.refine_abs_pose(pr["f"], pr["p"], T0[b], idx=idx, **okw)
            if not np.array_equal(Tr[b], wT) or iters[b] != wit:
                return params, "problem %d: refined pose bits / LM iterations (%d, oracle %d)" % (b, iters[b], wit)
    return params, None


def fuzz_relpose(ctx, rng):
    from test_oracle_relpose import _two_views
    P, S = int(rng.integers(1, 5)), int(rng.choice([16, 130, 600]))
    algorithm = int(rng.choice([5, 7, 8]))
    max_iter, adaptive, seed = int(rng.choice([1, 33, 200])), bool(rng.integers(0, 2)), int(rng.integers(0, 2 ** 31))
    thr = float(rng.choice([2.0 * (1.0 - np.cos(np.deg2rad(1.0))), 2.0 * (1.0 - np.cos(np.deg2rad(0.1))), 1e-12]))
    params = dict(P=P, S=S, algorithm=algorithm, max_iter=max_iter, adaptive=adaptive, seed=seed, thr=thr)
    problems = []
    for b in range(P):
        n = int(rng.integers(0, S + 1))
        a, c, _, _, _ = _two_views(rng, max(n, 1), noise_deg=float(rng.choice([0.0, 0.05, 0.5])), outlier_frac=float(rng.choice([0.0, 0.3, 0.9])))
        problems.append((a[:n], c[:n]))
    f1 = np.zeros((P, S, 3)); f2 = np.zeros((P, S, 3)); n_arr = np.zeros(P, np.int32)
    for b, (a, c) in enumerate(problems):
        n_arr[b] = a.shape[0]
        f1[b, :n_arr[b]], f2[b, :n_arr[b]] = a, c
    t1, t2, tn = _dev(ctx, f1, f2, n_arr)
    out = ctx.ransac_rel_pose(t1, t2, tn, thr, max_iter, algorithm=algorithm, seed=seed, adaptive=adaptive, want_counts=True)
    ctx.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for b, (a, c) in enumerate(problems):
        want = oracle.ransac_rel_pose(a, c, thr, max_iter, seed=seed + b, adaptive=adaptive, want_counts=True, algorithm=algorithm)
        used = want["iters_used"]
        if got["info"][b, 1] != used or got["info"][b, 0] != want["best_iter"] or got["info"][b, 2] != want["status"]:
            return params, "problem %d: iterations / winner / status" % b
        if not np.array_equal(got["counts"][b, :used], want["counts"][:used]):
            return params, "problem %d: hypothesis counts" % b
        if got["n_inliers"][b] != want["n_inliers"] or not np.array_equal(got["mask"][b, :n_arr[b]].astype(bool), want["mask"]):
            return params, "problem %d: inlier mask" % b
        if not np.array_equal(got["T"][b].view(np.uint64), want["T"].view(np.uint64)):
            return params, "problem %d: pose bits" % b
    return params, None


def fuzz_l2sort(ctx, rng):
    """float-descriptor matching (sosvo_match_l2) and the stable sort of match keys"""
    P, Sq, St, k = int(rng.integers(1, 6)), int(rng.choice([1, 50, 257])), int(rng.choice([1, 64, 300])), int(rng.integers(1, 3))
    D = int(rng.choice([32, 64, 128]))
    params = dict(P=P, q_stride=Sq, t_stride=St, k=k, dim=D)
    q = rng.integers(0, 8, (P, Sq, D)).astype(np.float32)   # small integers: exact sums, many ties
    t = rng.integers(0, 8, (P, St, D)).astype(np.float32)
    nq, nt = rng.integers(0, Sq + 1, P).astype(np.int32), rng.integers(0, St + 1, P).astype(np.int32)
    tq, tt, tnq, tnt = _dev(ctx, q, t, nq, nt)
    res = ctx.match_l2(tq, tt, tnq, tnt, k=k)
    # Hamming keys for the sort: random keys with many equal distances
    hk = (rng.integers(0, 6, (P, Sq, 1)).astype(np.uint32) << np.uint32(20)) | rng.integers(0, 1000, (P, Sq, 1)).astype(np.uint32)
    (thk,) = _dev(ctx, hk)
    order = ctx.sort_matches(thk, tnq)
    ctx.synchronize()
    res = res.cpu().numpy().view(np.uint64)
    order = order.cpu().numpy()
    for p in range(P):
        if nq[p] and not np.array_equal(res[p, :nq[p]], oracle.match_l2(q[p, :nq[p]], t[p, :nt[p]].reshape(-1, D), k=k)):
            return params, "problem %d: L2 matches" % p
        wo = oracle.sort_matches(hk[p, :nq[p]])
        if not np.array_equal(order[p, :nq[p]], wo):
            return params, "problem %d: sort order" % p
    return params, None


def fuzz_pipeline(ctx, rng):
    """Everything after detection (bucket matching, gates, triangulation, frame-to-frame matching, RANSAC, LM) on image-free
    frames against the reference's control flow on the oracle (tests/refflow.py)."""
    import refflow
    import synth
    from vo_single_camera_sos_amd.pipeline import FramePairPipeline, RigConfig
    B, NM = int(rng.integers(1, 5)), int(rng.choice([1, 4, 12]))
    cap = int(rng.choice([16, 64, 192]))
    frame_cap = int(rng.choice([256, 2048]))
    max_iter, adaptive = int(rng.choice([10, 100, 400])), bool(rng.integers(0, 2))
    solver = str(rng.choice(["P3P", "GP3P"]))
    rig_kw = dict(pano_top=synth.PANO_C2, pano_bot=synth.PANO_C2, F_top=synth.F_TOP, F_bot=synth.F_BOT,
                  min_range=float(rng.choice([0.0, 500.0, 2000.0])), max_range=float(rng.choice([3000.0, 7000.0, 1e9])),
                  stereo_min_disp=float(rng.choice([0.0, 1.0, 3.0])), stereo_max_hdiff=float(rng.choice([0.5, 2.5, 1e6])),
                  f2f_max_hdiff=float(rng.choice([-1.0, 10.0, 75.0])), pct_good_matches=float(rng.choice([1.0, 0.8, 0.3])))
    seed = int(rng.integers(0, 2 ** 31))
    params = dict(B=B, nmask=NM, bucket_cap=cap, frame_cap=frame_cap, max_iter=max_iter, adaptive=adaptive, solver=solver, seed=seed,
                  **{k: v for k, v in rig_kw.items() if isinstance(v, float)})
    frames = []
    for i in range(B):
        P, desc = synth.make_scene(rng, int(rng.choice([0, 30, 400, 1500])))
        R, t = synth.random_pose(rng)
        kw = dict(nmask=NM, cap=cap, flip_prob=float(rng.choice([0.0, 0.04, 0.2])), distractors=float(rng.choice([0.0, 0.15, 1.0])))
        frames.append(synth.observe_frame(rng, P, desc, np.eye(3), np.zeros(3), **kw))
        frames.append(synth.observe_frame(rng, P, desc, R, t, **kw))
    pipe = FramePairPipeline(ctx, RigConfig(**rig_kw), B, nmask=NM, bucket_cap=cap, frame_cap=frame_cap, max_iter=max_iter, adaptive=adaptive,
                             seed=seed, ransac_solver=solver)
    pipe.load_keypoints(synth.pack_buckets(frames, NM, cap))
    pipe.step()
    rec = pipe.results()
    ctx.synchronize()
    rec = rec.cpu().numpy()
    mask = pipe.ransac["mask"].cpu().numpy()
    M = pipe.frames["M"].cpu().numpy()
    rp = refflow.RigParams(**rig_kw)
    flagged = False
    for i in range(B):
        ref = refflow.stereo_frame(rp, *[frames[2 * i][k] for k in ("kp_top", "kp_bot", "desc_top", "desc_bot")])
        cur = refflow.stereo_frame(rp, *[frames[2 * i + 1][k] for k in ("kp_top", "kp_bot", "desc_top", "desc_bot")])
        if len(ref["X"]) > frame_cap or len(cur["X"]) > frame_cap:
            flagged = True     # more stereo points than the frame store holds: the first frame_cap in order are kept (sosvo.h)
            ref, cur = [{k: (v[:frame_cap] if k != "n_cand" else v) for k, v in fr.items()} for fr in (ref, cur)]
        if M[2 * i] != len(ref["X"]) or M[2 * i + 1] != len(cur["X"]):
            return params, "pair %d: stereo points (%d %d, oracle %d %d)" % (i, M[2 * i], M[2 * i + 1], len(ref["X"]), len(cur["X"]))
        w = refflow.track_pair(rp, ref, cur, pipe.thr, max_iter, seed=seed + i, adaptive=adaptive, gp3p=solver == "GP3P")
        n = len(w["corr"]["cam"])
        if rec[i, 13] != n:
            return params, "pair %d: correspondences (%d, oracle %d)" % (i, rec[i, 13], n)
        if rec[i, 14] != w["ransac"]["status"] or rec[i, 15] != w["ransac"]["best_iter"] or rec[i, 12] != w["ransac"]["n_inliers"]:
            return params, "pair %d: RANSAC status / winner / inliers" % i
        if not np.array_equal(mask[i, :n].astype(bool), w["ransac"]["mask"]):
            return params, "pair %d: inlier mask" % i
        if not np.array_equal(rec[i, :12].reshape(3, 4), w["T"]):
            return params, "pair %d: pose bits" % i
    return params, ("flagged" if flagged else None)


def _carved(ws, takes):
    """Host views of buffers a batch entry point leaves in its workspace: `takes` lists (name, count, dtype) in the order
    carve() / carve_rgbd() of pipeline.hip take them, each slice rounded up to 256 bytes, up to the last one wanted.  (A
    layout that drifted from the library's reads the random bytes the workspace was filled with: a mismatch, not a pass.)"""
    off, spans = 0, []
    for name, count, dt in takes:
        nb = int(count) * np.dtype(dt).itemsize
        spans.append((name, off, nb, dt))
        off += (nb + 255) & ~255
    host = ws[:off].cpu().numpy()
    return {name: host[o:o + nb].view(dt) for name, o, nb, dt in spans}


DETECTORS = ("GFT", "ORB", "FAST", "AGAST")
MEDIANS = (0, 1, 3, 5, 11)
BATCH_WIDTHS = (360, 480, 600, 720, 960, 1200)
BATCH_AZIMUTHS = (120.0, 45.0, 30.0, 15.0, 11.25)     # 3, 8, 12, 24, 32 azimuthal masks per mirror (32: the most a model holds)


def draw_batch(rng):
    """The parameters of one `batch` case (no GPU): a legal sosvo_batch_cfg for every detector.  GFT keeps at most 1024
    corners wanted (max_corners <= 1000) and minimum distances below the ~30 px at which the third-of-a-cell overflow list
    can fill, so its only documented overflow is the candidate limit (status bit 0: the strongest candidates are kept, which
    the oracle's flow restates)."""
    det = str(rng.choice(DETECTORS))
    d = dict(detector=det, median=int(rng.choice(MEDIANS)), width=int(rng.choice(BATCH_WIDTHS)),
             azimuth=float(rng.choice(BATCH_AZIMUTHS)), n_pairs=int(rng.integers(1, 6)),
             frame_cap=int(rng.choice([48, 256, 2048])), quality=0.01, min_distance=5.0,
             solver=str(rng.choice(["P3P", "GP3P"])), max_iter=int(rng.choice([10, 100, 400])), adaptive=bool(rng.integers(0, 2)),
             pattern=str(rng.choice(["opencv", "seeded"])), seed=int(rng.integers(0, 2 ** 31)))
    if det == "GFT":
        d["kp_cap"] = int(rng.choice([16, 64, 256, 1024, 1088, 2048]))
        d["max_corners"] = int(rng.choice([7, 50, 300, 1000]))
        d["quality"] = float(10 ** rng.uniform(-3, -0.5))
        d["min_distance"] = float(rng.choice([0.7, 1.0, 2.5, 5.0, 7.5, 12.0]))
    elif det == "ORB":
        d["kp_cap"] = int(rng.choice([16, 64, 256, 1024, 2048]))
        d["max_corners"] = int(rng.choice([10, 60, 250, 1000, 2500]))
    else:
        d["kp_cap"] = int(rng.choice([16, 64, 512, 2048, 4096]))
        d["max_corners"] = int(rng.choice([50, 1000]))
    d["n_streams"] = int(rng.integers(1, min(4, d["n_pairs"]) + 1))
    d["frames"] = [(int(rng.integers(0, _POOL_PAIRS)), int(rng.integers(0, 5)), int(rng.integers(0, 2 ** 31)))
                   for _ in range(d["n_pairs"])]
    return d


_POOL_PAIRS = 4
_BATCH_CACHE = {}


def _batch_model(ctx, width, azimuth):
    """(DeviceImageModel, rig kwargs, host tables) of the synthetic rig at one panorama width and mask count, built once per
    process; the omni frames (rendered once) do not depend on either."""
    from vo_single_camera_sos_amd import synthetic
    from vo_single_camera_sos_amd.frontend import DeviceImageModel
    from vo_single_camera_sos_amd.omnistereo.gum import synthetic_gums
    from vo_single_camera_sos_amd.omnistereo.panorama import Panorama
    key = (width, azimuth)
    if key not in _BATCH_CACHE:
        gs = synthetic_gums()
        for m in (gs.top_model, gs.bot_model):
            m.panorama = Panorama(m, width=width)
        gs.make_annulus_masks((480, 640))
        if "omni" not in _BATCH_CACHE:
            _BATCH_CACHE["omni"] = synthetic.make_frame_pairs(gs, _POOL_PAIRS, seed=5150)[0]
        model = DeviceImageModel(ctx, gs, (480, 640), azimuth_mask_degrees=azimuth)
        model.unwrap_table = ctx.unwrap_prepare(model.omni_masks, model.map_x, model.map_y, (model.H, model.W))
        pano = gs.top_model.panorama
        geo = (pano.cols, pano.rows, pano.pixel_size, pano.cyl_height_max)
        rig_kw = dict(pano_top=geo, pano_bot=geo, F_top=gs.top_model.F[:3, 0], F_bot=gs.bot_model.F[:3, 0], min_range=500.0,
                      max_range=7000.0, stereo_min_disp=1.0, stereo_max_hdiff=2.5, f2f_max_hdiff=0.125 * 0.5 * pano.cols,
                      pct_good_matches=1.0)
        host = (model.map_x.cpu().numpy(), model.map_y.cpu().numpy(), model.omni_masks.cpu().numpy())
        _BATCH_CACHE[key] = (model, rig_kw, host)
    return _BATCH_CACHE[key]


def _perturb(omni_pair, kind, seed):
    """a pooled frame pair, perturbed: 0 as rendered, 1 noise, 2 the current frame shifted, 3 a black frame, 4 a saturated one"""
    r = np.random.default_rng(seed)
    pair = omni_pair.copy()
    if kind == 1:
        pair = np.clip(pair.astype(np.int16) + r.normal(0, r.uniform(1, 8), pair.shape).round().astype(np.int16), 0, 255).astype(np.uint8)
    elif kind == 2:
        pair[1] = np.roll(pair[1], (int(r.integers(-6, 7)), int(r.integers(-6, 7))), axis=(0, 1))
    elif kind == 3:
        pair[int(r.integers(0, 2))] = 0
    elif kind == 4:
        pair[int(r.integers(0, 2))] = 255
    return pair


def fuzz_batch(ctx, rng):
    """The omni one-call batch (sosvo_frame_pair_batch: unwrap, median, detection with any of the four detectors,
    descriptors, static stereo, frame-to-frame matching, RANSAC, LM) driven from rendered frames, on a dirty workspace,
    against the reference's control flow on the oracle (oracle/flow.py, tests/refflow.py): every pair's record, inlier mask and stereo point
    counts bit for bit; the same batch through sosvo_frame_pair_batch_streams gives the same records."""
    import ctypes
    import refflow
    from vo_single_camera_sos_amd import _lib
    from vo_single_camera_sos_amd.pipeline import RigConfig
    d = draw_batch(rng)
    params = {k: v for k, v in d.items() if k != "frames"}
    model, rig_kw, (mx, my, om) = _batch_model(ctx, d["width"], d["azimuth"])
    B, NM = d["n_pairs"], model.nmask
    params["nmask"], params["rows"], params["cols"] = NM, model.rows, model.cols
    pool = _BATCH_CACHE["omni"]
    omni = np.concatenate([_perturb(pool[2 * i:2 * i + 2], k, sd) for i, k, sd in d["frames"]])
    pat_host = orb_pattern.orb_pattern(d["pattern"])
    ca, sa = orb_pattern.angle_cos_sin(orb_pattern.GFT_KEYPOINT_ANGLE)
    c = _lib.BatchCfg()
    c.n_pairs, c.H, c.W, c.rows, c.cols, c.nmask = B, model.H, model.W, model.rows, model.cols, NM
    c.kp_cap, c.frame_cap, c.median_ksize, c.max_corners, c.edge = d["kp_cap"], d["frame_cap"], d["median"], d["max_corners"], 31
    c.ransac_max_iter, c.ransac_adaptive, c.lm_max_iter = d["max_iter"], int(d["adaptive"]), 30
    c.quality, c.min_distance = d["quality"], d["min_distance"]
    thr = float(1.0 - np.cos(np.deg2rad(5.0)))
    c.ransac_threshold, c.seed, c.cos_a, c.sin_a = thr, d["seed"], float(ca), float(sa)
    c.ransac_flags, c.detector = (_lib.FLAG_GP3P if d["solver"] == "GP3P" else 0), _lib.DETECTORS[d["detector"]]
    rig = RigConfig(**rig_kw).as_struct()
    t_omni, t_pat = _dev(ctx, omni, pat_host)
    ws = torch.empty((ctx.frame_pair_batch_workspace(c),), dtype=torch.uint8, device=ctx.device)
    ws.fill_(int(rng.integers(0, 256)))
    ctx.debug_fill_scratch(int(rng.integers(0, 256)))
    rec = ctx.frame_pair_batch(rig, c, t_omni, model.unwrap_table, model.mask_bits, t_pat, ws)
    ctx.synchronize()
    rec = rec.cpu().numpy()
    # the same batch split over internal streams (n_streams = 1 included), on its own dirty workspace
    ns = d["n_streams"]
    ws2 = torch.empty((ctx.frame_pair_batch_streams_workspace(c, ns),), dtype=torch.uint8, device=ctx.device)
    ws2.fill_(int(rng.integers(0, 256)))
    rec2 = torch.full((B, 16), float("nan"), dtype=torch.float64, device=ctx.device)
    cp = lambda x: ctypes.cast(ctypes.pointer(x), ctypes.c_void_p)  # noqa: E731
    ctx._call(ctx._lib.sosvo_frame_pair_batch_streams, cp(rig), cp(c), ns, t_omni.data_ptr(), model.unwrap_table.data_ptr(),
              model.mask_bits.data_ptr(), t_pat.data_ptr(), ws2.data_ptr(), ws2.numel(), rec2.data_ptr())
    ctx.synchronize()
    if not np.array_equal(rec2.cpu().numpy().view(np.uint64), rec.view(np.uint64)):
        return params, "n_streams %d: records differ from the single call's" % ns
    F, Fc = 2 * B, d["frame_cap"]
    NI, P, cap, Cc = 2 * F, 2 * F * NM, d["kp_cap"], 2 * Fc
    w = _carved(ws, [("gray", NI * model.rows * model.cols, np.uint8), ("kp", P * cap * 2, np.float32), ("n", P, np.int32),
                     ("status", P, np.int32), ("desc", P * cap * 32, np.uint8), ("s_keys", P // 2 * cap, np.uint32),
                     ("s_order", P // 2 * cap, np.int32), ("n_cand", F, np.int32), ("gray_rows", 4, np.int32),
                     ("m_top", F * Fc * 2, np.float32), ("m_bot", F * Fc * 2, np.float32),
                     ("d_top", F * Fc * 32, np.uint8), ("d_bot", F * Fc * 32, np.uint8), ("X", F * Fc * 3, np.float64),
                     ("b_top", F * Fc * 3, np.float64), ("b_bot", F * Fc * 3, np.float64), ("M", F, np.int32),
                     ("ref_frame", B, np.int32), ("cur_frame", B, np.int32),
                     ("k_top", B * Fc, np.uint32), ("k_bot", B * Fc, np.uint32), ("o_top", B * Fc, np.int32),
                     ("o_bot", B * Fc, np.int32), ("f", B * Cc * 3, np.float64), ("p", B * Cc * 3, np.float64),
                     ("cam", B * Cc, np.int32), ("cq", B * Cc, np.int32), ("ct", B * Cc, np.int32), ("cn", B, np.int32),
                     ("cn_top", B, np.int32), ("T_ransac", B * 12, np.float64), ("mask", B * Cc, np.uint8)])
    status = w["status"].reshape(NI, NM)
    M, mask = w["M"], w["mask"].reshape(B, Cc)
    im = refflow.ImageModel(mx, my, om, model.mask_bits_host, NM, d["max_corners"], pat_host, ca, sa, median_ksize=d["median"],
                            quality=d["quality"], min_distance=d["min_distance"], method=d["detector"], kp_cap=cap)
    rp = refflow.RigParams(**rig_kw)
    flagged = False
    for i in range(B):
        skip = False
        frames = []
        for f in (2 * i, 2 * i + 1):
            imgs = (f, F + f)     # view-major images: top mirror of frame f, bottom mirror of frame f
            if d["detector"] == "GFT" and (status[list(imgs)] & 2).any():
                skip = True       # a mask's cell grid does not fit on chip (status bit 1); bit 0 alone is a defined result:
                                  # the strongest candidates are kept, and flow.detect_view cuts its list the same way
            if d["detector"] == "AGAST":
                for v, img in enumerate(imgs):
                    pano = oracle.unwrap(omni[f], om[v], mx[v], my[v])
                    over = int((oracle.fast_score_map(oracle.median_gray(pano, d["median"]), 10) > 0).sum()) > 16384
                    if bool((status[img] & 2).any()) != over or (over and not (status[img] & 2).all()):
                        return params, "pair %d frame %d view %d: AGAST overflow flag (%s, oracle %s)" % (i, f, v, status[img].tolist(), over)
                    skip |= over  # more than 16384 FAST corners before AGAST's suppression: the rest is dropped (sosvo.h)
            if not skip:     # refflow.frame_from_image on the detection flow of oracle/flow.py
                (kt, dt, _, _), (kb, db, _, _) = flow.detect_view(im, omni[f], 0), flow.detect_view(im, omni[f], 1)
                frames.append(refflow.stereo_frame(rp, kt, kb, dt, db))
        if skip:
            flagged = True
            continue
        for k, fr in enumerate(frames):
            if len(fr["X"]) > Fc:
                flagged = True     # more stereo points than the frame store holds: the first frame_cap in order are kept (sosvo.h)
                frames[k] = {key: (v[:Fc] if key not in ("n_cand", "n_kp_top", "n_kp_bot") else v) for key, v in fr.items()}
        ref, cur = frames
        if M[2 * i] != len(ref["X"]) or M[2 * i + 1] != len(cur["X"]):
            return params, "pair %d: stereo points (%d %d, oracle %d %d)" % (i, M[2 * i], M[2 * i + 1], len(ref["X"]), len(cur["X"]))
        wt = refflow.track_pair(rp, ref, cur, thr, d["max_iter"], seed=d["seed"] + i, adaptive=d["adaptive"], gp3p=d["solver"] == "GP3P")
        n = len(wt["corr"]["cam"])
        want = np.concatenate([np.asarray(wt["T"], np.float64).reshape(12), [wt["ransac"]["n_inliers"], n, wt["ransac"]["status"],
                                                                             wt["ransac"]["best_iter"]]])
        if not np.array_equal(rec[i].view(np.uint64), want.view(np.uint64)):
            return params, "pair %d: record %s, oracle %s" % (i, rec[i, 12:].tolist(), want[12:].tolist())
        if not np.array_equal(mask[i, :n].astype(bool), wt["ransac"]["mask"]):
            return params, "pair %d: inlier mask" % i
    return params, ("flagged" if flagged else None)


RGBD_KP_CAPS = {"GFT": (64, 512, 1024, 1088, 2048), "ORB": (64, 512, 1024, 1536, 2048), "FAST": (64, 1024, 1088, 4096),
                "AGAST": (64, 1024, 1088, 4096)}


def draw_rgbd(rng):
    """The parameters of one `rgbd` case (no GPU): a legal sosvo_rgbd_batch_cfg, the detector in flags bits 8-9, kp_cap on
    both sides of 1024 (GFT's whole-image variant starts above it; ORB up to 2048).  GFT wants at most 1000 corners."""
    det = str(rng.choice(DETECTORS))
    d = dict(detector=det, B=int(rng.integers(1, 4)), rows=int(rng.integers(80, 200)), cols=int(rng.integers(100, 320)),
             kp_cap=int(rng.choice(RGBD_KP_CAPS[det])), nfeat=int(rng.choice([50, 400, 1000] if det == "GFT" else [50, 400, 2000])),
             algo=str(rng.choice(["EPNP", "KNEIP", "GP3P", "TWOPT"])), depth_is_Z=bool(rng.integers(0, 2)),
             ksize=int(rng.choice([0, 0, 1, 3, 5, 11])), max_iter=int(rng.choice([20, 200])), adaptive=bool(rng.integers(0, 2)),
             seed=int(rng.integers(0, 2 ** 31)), thr=float(rng.choice([1.0 - np.cos(np.deg2rad(5.0)), 1.0 - np.cos(np.deg2rad(0.5))])))
    d["frame_cap"] = int(rng.choice([d["kp_cap"], d["kp_cap"], 32, 200]))
    return d


def rgbd_frames(rng, B, rows, cols):
    """B random RGB-D pairs (no GPU): a texture shifted between the two frames of a pair; depth in metres (the units of the
    0.8 .. 7 m range gates) on 8x8 blocks, some beyond the gates, with holes of 0 or NaN -> bgr [2B,rows,cols,3] u8,
    depth [2B,rows,cols] f32"""
    bgr, depth = [], []
    for i in range(B):
        base = np.stack([_image(rng, rows + 8, cols + 8, int(rng.integers(0, 2))) for _ in range(3)], axis=-1)
        dz = rng.uniform(0.5, 9.0, (rows + 8, cols + 8)).astype(np.float32)
        dz = np.kron(dz[::8, ::8], np.ones((8, 8), np.float32))[:rows + 8, :cols + 8]
        sx, sy = int(rng.integers(0, 8)), int(rng.integers(0, 8))
        for (ox, oy) in ((0, 0), (sx, sy)):
            im = np.ascontiguousarray(base[oy:oy + rows, ox:ox + cols])
            d = np.array(dz[oy:oy + rows, ox:ox + cols], np.float32)
            hole = rng.random((rows, cols)) < float(rng.choice([0.0, 0.1, 0.9]))
            d[hole] = float(rng.choice([0.0, np.nan]))
            bgr.append(im)
            depth.append(d)
    return np.stack(bgr), np.stack(depth)


def fuzz_rgbd(ctx, rng):
    """The RGB-D (perspective) path behind ONE C-ABI call (sosvo_rgbd_pair_batch) on small random frames with any of the four
    detectors -- textures shifted between the frames of a pair, depth maps with holes / NaN / out-of-range values, both
    depth conventions, all solvers, an optional median window, capacities on both sides of 1024 and frame caps that cut --
    on a dirty workspace, against the reference's control flow on the oracle (oracle/flow.py, tests/refflow.py)."""
    import refflow
    from vo_single_camera_sos_amd import _lib
    from vo_single_camera_sos_amd.pipeline import RGBDCamConfig, RGBDPairBatch
    d = draw_rgbd(rng)
    params = dict(d)
    B, rows, cols, nfeat, algo, ksize = d["B"], d["rows"], d["cols"], d["nfeat"], d["algo"], d["ksize"]
    depth_is_Z, max_iter, adaptive, seed, thr, det = d["depth_is_Z"], d["max_iter"], d["adaptive"], d["seed"], d["thr"], d["detector"]
    cap, Fc = d["kp_cap"], d["frame_cap"]
    fx, fy, cx, cy = 0.8 * cols, 0.8 * cols, 0.5 * cols - 0.5, 0.5 * rows - 0.5
    bgr, depth = rgbd_frames(rng, B, rows, cols)
    cam = RGBDCamConfig(fx=fx, fy=fy, center_x=cx, center_y=cy, depth_is_Z=depth_is_Z, min_range=0.8, max_range=7.0)
    one = RGBDPairBatch(ctx, cam, B, image_shape=(rows, cols), num_of_features=nfeat, kp_cap=cap, frame_cap=Fc, max_iter=max_iter,
                        adaptive=adaptive, seed=seed, thr=thr, pose_est_algorithm=algo, median_win_size=ksize, detection_method=det)
    assert one.cfg.flags >> 8 == _lib.DETECTORS[det] and one.cfg.kp_cap == cap and one.cfg.frame_cap == Fc
    one.workspace.fill_(int(rng.integers(0, 256)))
    ctx.debug_fill_scratch(int(rng.integers(0, 256)))
    one.load_frames(bgr, depth)
    rec = one.step()
    ctx.synchronize()
    rec = rec.cpu().numpy()
    F = 2 * B
    w = _carved(one.workspace, [("gray", F * rows * cols, np.uint8), ("kp", F * cap * 2, np.float32), ("n", F, np.int32),
                                ("status", F, np.int32), ("desc", F * cap * 32, np.uint8), ("m", F * Fc * 2, np.float32),
                                ("d", F * Fc * 32, np.uint8), ("X", F * Fc * 3, np.float64), ("b", F * Fc * 3, np.float64),
                                ("M", F, np.int32)])
    ca, sa = orb_pattern.angle_cos_sin(orb_pattern.GFT_KEYPOINT_ANGLE)
    rc = refflow.RGBDParams(fx, fy, cx, cy, cam.focal_length_m, depth_is_Z, 0.8, 7.0, cam.f2f_max_hdiff, 1.0)
    pat = orb_pattern.orb_pattern()
    flagged = False
    for i in range(B):
        skip = False
        for f in (2 * i, 2 * i + 1):
            if det == "GFT" and w["status"][f] & 2:
                skip = True       # the cell grid does not fit on chip (status bit 1); bit 0 alone is a defined result: the
                                  # strongest candidates are kept, and flow.rgbd_frame cuts its list the same way
            if det == "AGAST":
                over = int((oracle.fast_score_map(oracle.median_gray(bgr[f], ksize), 10) > 0).sum()) > 16384
                if bool(w["status"][f] & 2) != over:
                    return params, "frame %d: AGAST overflow flag (%d, oracle %s)" % (f, w["status"][f], over)
                skip |= over
        if skip:
            flagged = True
            continue
        frames = []
        for f in (2 * i, 2 * i + 1):
            fr = flow.rgbd_frame(rc, bgr[f], depth[f], nfeat, pat, ca, sa, median_ksize=ksize, method=det, kp_cap=cap)
            if len(fr["X"]) > Fc:
                flagged = True     # more keypoints with valid depth than the frame store holds: the first frame_cap are kept
                fr = {k: (v[:Fc] if k != "n_kp" else v) for k, v in fr.items()}
            if w["M"][f] != len(fr["X"]):
                return params, "frame %d: keypoints with depth (%d, oracle %d)" % (f, w["M"][f], len(fr["X"]))
            frames.append(fr)
        wt = refflow.track_pair_rgbd(rc, frames[0], frames[1], thr, max_iter, seed=seed + i, adaptive=adaptive,
                                     epnp=(algo == "EPNP"), gp3p=(algo == "GP3P"), twopt=(algo == "TWOPT"))
        n = len(wt["corr"]["q"])
        if rec[i, 13] != n:
            return params, "pair %d: correspondences (%d, oracle %d)" % (i, rec[i, 13], n)
        if rec[i, 14] != wt["ransac"]["status"] or rec[i, 15] != wt["ransac"]["best_iter"] or rec[i, 12] != wt["ransac"]["n_inliers"]:
            return params, "pair %d: RANSAC status / winner / inliers (%s, oracle %d %d %d)" % (
                i, rec[i, 12:16].tolist(), wt["ransac"]["n_inliers"], wt["ransac"]["status"], wt["ransac"]["best_iter"])
        if not np.array_equal(rec[i, :12].reshape(3, 4), wt["T"]):
            return params, "pair %d: pose bits" % i
    return params, ("flagged" if flagged else None)


STAGES = {"median": fuzz_median, "gft": fuzz_gft, "fast": fuzz_fast, "agast": fuzz_agast, "match": fuzz_match,
          "radius": fuzz_radius, "orb": fuzz_orb, "unwrap": fuzz_unwrap, "ransac": fuzz_ransac,
          "describe": fuzz_describe, "relpose": fuzz_relpose, "l2sort": fuzz_l2sort,
          "pipeline": fuzz_pipeline, "rgbd": fuzz_rgbd, "batch": fuzz_batch, "cross_check": fuzz_cross_check,
          "gated_match": fuzz_gated_match}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=5.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--stages", default=",".join(STAGES))
    ap.add_argument("--first-case", type=int, default=0)
    ap.add_argument("--cases", type=int, default=0, help="stop after this many cases per stage (0 = by time)")
    args = ap.parse_args()
    oracle.build()
    ctx = Context(0)
    stages = [s for s in args.stages.split(",") if s]
    t_end = time.time() + 60 * args.minutes
    done = {s: 0 for s in stages}
    flagged = {s: 0 for s in stages}
    refused = {s: 0 for s in stages}
    messages = set()
    case = args.first_case
    t_print = time.time()
    while time.time() < t_end and (args.cases == 0 or case < args.first_case + args.cases):
        for s in stages:
            rng = np.random.default_rng([args.seed, list(STAGES).index(s), case])
            try:
                params, err = STAGES[s](ctx, rng)
            except SosvoError as e:     # an argument the entry point refuses: not a case (the run cannot end "all identical")
                refused[s] += 1
                msg = str(e).split(":")[-1].strip()
                if msg not in messages:
                    messages.add(msg)
                    print("refused (stage %s case %d): %s" % (s, case, e), flush=True)
                continue
            if err == "flagged":
                flagged[s] += 1
            elif err:
                print("MISMATCH stage %s case %d (seed %d): %s\n  %s" % (s, case, args.seed, err, params), flush=True)
                return 1
            done[s] += 1
        case += 1
        if time.time() - t_print > 20:
            t_print = time.time()
            print("cases %s flagged %s" % (done, flagged), flush=True)
    # a draw the ABI refused, or --minutes ending the run before --cases, leaves stages short: say so and fail
    short = {s: n for s, n in done.items() if (args.cases and n < args.cases) or n == 0}
    if short or any(refused.values()):
        print("fuzz_parity: INCOMPLETE (short %s, refused %s).  cases %s flagged %s seed %d first-case %d" % (
            short, {s: n for s, n in refused.items() if n}, done, flagged, args.seed, args.first_case), flush=True)
        return 2
    print("fuzz_parity: all identical.  cases %s flagged %s seed %d first-case %d" % (done, flagged, args.seed, args.first_case), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
