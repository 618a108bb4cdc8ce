#!/usr/bin/env python
"""What the stage entry points whose hosts share a body or a set of checks answer to a wrong argument: a characterisation
sweep over raw ctypes calls.  geometry.hip's six assemble entry points, the two gray pyramids, sosvo_track_lk,
sosvo_refine_stereo_lk, the gated / gated-cyclic / ratio matchers and the dense four.

Every case starts from arguments the entry point accepts (one small device buffer stands behind every pointer) and makes one
of them wrong, or two, to pin which check speaks first.  Nothing is launched: where an entry point returns SOSVO_OK early on
empty input the accepted arguments ARE the empty input (a case that breaks no rule ends there; the sizes a check reads are
set by the case), and every case of the dense four, which have no empty input, breaks a rule.  An outcome is (entry point,
case, status, message of sosvo_last_error; "" with SOSVO_OK).

    python scripts/record_abi_messages.py tests/golden/abi_messages_parent.json

writes the outcomes of the tree it is run from (it needs a GPU: a context is created); tests/test_gpu_abi_messages.py
recomputes them and compares.  The committed file was written from the commit BEFORE the entry points' hosts were merged, by
this script unchanged."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from vo_single_camera_sos_amd import _lib  # noqa: E402

NAN = float("nan")
c_p, c_i32 = ctypes.c_void_p, ctypes.c_int32


def _rig(w_top=1200.0, w_bot=1200.0):
    r = _lib.Rig()
    r.pano_top[:] = [w_top, 300.0, 0.005, 1.2]
    r.pano_bot[:] = [w_bot, 300.0, 0.005, 1.2]
    r.F_top[:] = [0.0, 0.0, 100.0]
    r.F_bot[:] = [0.0, 0.0, -100.0]
    r.min_range, r.max_range = 500.0, 7000.0
    return r


def table(P, keep):
    """-> [(entry point, parameter names, accepted values, [(case, overrides)])].  P: a device pointer, 256-byte aligned, with
    a few dozen bytes behind it; keep: what must outlive the calls (host structs)."""
    def host(obj):
        keep.append(obj)
        return ctypes.addressof(obj)
    rig, rig_half, rig_bot = host(_rig()), host(_rig(1200.5)), host(_rig(1200.0, 0.0))
    rig_differs = host(_rig(1200.0, 1204.0))
    slk_bad = host(_lib.StereoLkOptionsStruct(11, 10, 0.01, 1e-4, 0.0))
    slots = host((c_i32 * 2)(0, 1))
    out = []

    stereo = ("rig kp_top kp_bot desc_top desc_bot n_top n_bot keys order nframes nmask cap out_cap m_top m_bot d_top d_bot X "
              "b_top b_bot M n_cand")
    stereo_ok = dict({n: P for n in stereo.split()}, rig=rig, nframes=0, nmask=3, cap=8, out_cap=16)
    stereo_cases = [("kp_top_null", dict(kp_top=0)), ("order_null", dict(order=0)), ("M_null", dict(M=0)), ("n_cand_null", dict(n_cand=0)),
                    ("nframes_negative", dict(nframes=-1)), ("nmask_0", dict(nmask=0)), ("out_cap_0", dict(out_cap=0)),
                    ("cap_above_keys", dict(cap=(1 << 20) + 1)), ("empty", {}), ("nframes_above", dict(nframes=(1 << 20) + 1)),
                    ("rig_null+M_null", dict(rig=0, M=0)), ("M_null+nmask_0", dict(M=0, nmask=0)), ("cap_0+cap_above", dict(cap=(1 << 20) + 1, out_cap=0))]
    out.append(("sosvo_stereo_assemble", stereo, stereo_ok, stereo_cases))
    s_names = stereo.replace("nframes nmask", "nframes slot_of_frame nmask")
    out.append(("sosvo_stereo_assemble_slots", s_names, dict(stereo_ok, slot_of_frame=slots),
                stereo_cases + [("slots_null", dict(slot_of_frame=0)), ("slots_null+M_null", dict(slot_of_frame=0, M=0))]))

    f2f = ("rig m_top m_bot X b_top b_bot M frame_cap ref_frame cur_frame keys_top order_top keys_bot order_bot npairs corr_cap "
           "f p cam corr_q corr_t n n_topview")
    f2f_ok = dict({n: P for n in f2f.split()}, rig=rig, frame_cap=16, npairs=0, corr_cap=32)
    f2f_cases = [("m_top_null", dict(m_top=0)), ("cur_frame_null", dict(cur_frame=0)), ("keys_top_null", dict(keys_top=0)), ("n_null", dict(n=0)),
                 ("npairs_negative", dict(npairs=-1)), ("frame_cap_0", dict(frame_cap=0)), ("corr_cap_0", dict(corr_cap=0)),
                 ("empty", {}), ("npairs_above", dict(npairs=(1 << 20) + 1)), ("n_topview_null", dict(n_topview=0)),
                 ("period_half", dict(rig=rig_half)), ("period_bot_0", dict(rig=rig_bot)),
                 ("rig_null+n_null", dict(rig=0, n=0)), ("n_null+corr_cap_0", dict(n=0, corr_cap=0)),
                 ("corr_cap_0+period_half", dict(corr_cap=0, rig=rig_half))]
    out.append(("sosvo_f2f_assemble", f2f, f2f_ok, f2f_cases))
    out.append(("sosvo_f2f_assemble_cyclic", f2f, f2f_ok, f2f_cases))
    trk = "rig m_top m_bot X M frame_cap ref_frame trk_top trk_bot st_top st_bot npairs corr_cap f p cam corr_q corr_t n n_topview"
    trk_ok = dict({n: P for n in trk.split()}, rig=rig, frame_cap=16, npairs=0, corr_cap=32)
    trk_cases = [("trk_top_null", dict(trk_top=0)), ("st_bot_null", dict(st_bot=0)), ("f_null", dict(f=0)), ("n_null", dict(n=0)),
                 ("npairs_negative", dict(npairs=-1)), ("frame_cap_0", dict(frame_cap=0)), ("corr_cap_0", dict(corr_cap=0)),
                 ("empty", {}), ("npairs_above", dict(npairs=(1 << 20) + 1)), ("n_topview_null", dict(n_topview=0)),
                 ("period_half", dict(rig=rig_half)), ("period_bot_0", dict(rig=rig_bot)),
                 ("rig_null+n_null", dict(rig=0, n=0)), ("n_null+corr_cap_0", dict(n=0, corr_cap=0)),
                 ("corr_cap_0+period_half", dict(corr_cap=0, rig=rig_half))]
    out.append(("sosvo_f2f_assemble_tracked", trk, trk_ok, trk_cases))
    out.append(("sosvo_f2f_assemble_tracked_cyclic", trk, trk_ok, trk_cases))

    pyr = "gray nimg rows cols levels row_range pyr"
    pyr_ok = dict(gray=P, nimg=0, rows=24, cols=32, levels=3, row_range=0, pyr=P)
    pyr_cases = [("gray_null", dict(gray=0)), ("levels_5", dict(levels=5)), ("levels_0", dict(levels=0)), ("rows_0", dict(rows=0)),
                 ("cols_16385", dict(cols=16385)), ("nimg_negative", dict(nimg=-1)), ("cols_30", dict(cols=30)), ("nimg_65536", dict(nimg=65536)),
                 ("pyr_null", dict(pyr=0)), ("pyr_null_level_1", dict(pyr=0, levels=1)),
                 ("row_range_odd", dict(row_range=P, nimg=3)), ("empty", {}),
                 ("gray_null+levels_5", dict(gray=0, levels=5)), ("cols_30+pyr_null", dict(cols=30, pyr=0)),
                 ("cols_30+levels_5", dict(cols=30, levels=5)), ("pyr_null+row_range_odd", dict(pyr=0, row_range=P, nimg=3))]
    out.append(("sosvo_gray_pyramid", pyr, pyr_ok, pyr_cases))
    out.append(("sosvo_gray_pyramid_cyclic", pyr, pyr_ok, pyr_cases))

    lk = ("gray pyr nimg rows cols levels row_range prev_img next_img nprob cap prev_pts n half max_iter eps min_eig flags next_pts "
          "status err back fb_max")
    lk_ok = dict({n: P for n in lk.split()}, nimg=2, rows=24, cols=32, levels=2, row_range=0, nprob=0, cap=8, half=3, max_iter=10, eps=0.01,
                 min_eig=1e-4, flags=0, back=0, fb_max=0.0)
    out.append(("sosvo_track_lk", lk, lk_ok, [
        ("gray_null", dict(gray=0)), ("err_null", dict(err=0)), ("levels_5", dict(levels=5)), ("rows_16385", dict(rows=16385)),
        ("pyr_null", dict(pyr=0)), ("pyr_null_level_1", dict(pyr=0, levels=1)), ("row_range_odd", dict(row_range=P, nimg=3)),
        ("nprob_negative", dict(nprob=-1)), ("nprob_65536", dict(nprob=65536)), ("cap_0", dict(cap=0)), ("cap_4097", dict(cap=4097)),
        ("half_1", dict(half=1)), ("half_11", dict(half=11)), ("max_iter_0", dict(max_iter=0)), ("max_iter_31", dict(max_iter=31)),
        ("eps_negative", dict(eps=-1.0)), ("min_eig_nan", dict(min_eig=NAN)), ("flag_2", dict(flags=2)), ("flag_8", dict(flags=8)),
        ("cyclic_cols_30", dict(flags=4, cols=30, levels=3)), ("cyclic_top_level_narrow", dict(flags=5, cols=32, levels=3, half=5)),
        ("back_without_fb_max", dict(back=P)), ("back_fb_max_nan", dict(back=P, fb_max=NAN)),
        ("empty", {}), ("no_images", dict(nimg=0)), ("cyclic", dict(flags=4)), ("back_fb_max", dict(back=P, fb_max=1.0)),
        ("gray_null+levels_5", dict(gray=0, levels=5)), ("nprob_negative+cap_0", dict(nprob=-1, cap=0)), ("half_11+max_iter_0", dict(half=11, max_iter=0)),
        ("eps_negative+flag_2", dict(eps=-1.0, flags=2)), ("cyclic_cols_30+back_without_fb_max", dict(flags=4, cols=30, levels=3, back=P)),
        ("flag_2+cyclic_cols_30", dict(flags=6, cols=30, levels=3))]))

    slk = "gray nimg rows cols row_range nmask cap kp_top n_top kp_bot n_bot keys stereo_min_disp stereo_max_hdiff options status"
    slk_ok = dict({n: P for n in slk.split()}, nimg=0, rows=24, cols=32, row_range=0, nmask=1, cap=16, stereo_min_disp=0.0,
                  stereo_max_hdiff=2.0, options=0, status=0)
    out.append(("sosvo_refine_stereo_lk", slk, slk_ok, [
        ("gray_null", dict(gray=0)), ("keys_null", dict(keys=0)), ("nimg_odd", dict(nimg=3)), ("rows_0", dict(rows=0)), ("nmask_0", dict(nmask=0)),
        ("cap_4097", dict(cap=4097)), ("problems_65536", dict(nimg=2 * 4096, nmask=16)), ("half_11", dict(options=slk_bad)),
        ("min_disp_nan", dict(stereo_min_disp=NAN)), ("max_hdiff_nan", dict(stereo_max_hdiff=NAN)), ("empty", {}), ("nimg_65536", dict(nimg=65536)),
        ("keys_null+nimg_odd", dict(keys=0, nimg=3)), ("nimg_odd+cap_0", dict(nimg=3, cap=0)), ("cap_0+half_11", dict(cap=0, options=slk_bad)),
        ("half_11+min_disp_nan", dict(options=slk_bad, stereo_min_disp=NAN))]))

    gated = "q_desc t_desc q_pos t_pos nq nt q_slot t_slot nprob n_forward q_stride t_stride min_dv max_du max_distance keys"
    gated_ok = dict({n: P for n in gated.split()}, q_slot=0, t_slot=0, nprob=0, n_forward=0, q_stride=8, t_stride=8, min_dv=0.0, max_du=2.0,
                    max_distance=64)
    sizes = [("nprob_negative", dict(nprob=-1)), ("nprob_65536", dict(nprob=65536)), ("n_forward_above", dict(n_forward=1)),
             ("n_forward_negative", dict(n_forward=-1)), ("q_stride_0", dict(q_stride=0)), ("q_stride_above_keys", dict(q_stride=(1 << 20) + 1)),
             ("t_stride_0", dict(t_stride=0)), ("nprob_negative+q_stride_0", dict(nprob=-1, q_stride=0)),
             ("n_forward_above+t_stride_0", dict(n_forward=1, t_stride=0))]
    gated_cases = [("q_pos_null", dict(q_pos=0)), ("keys_null", dict(keys=0)), ("nt_null", dict(nt=0))] + sizes + [
        ("max_distance_257", dict(max_distance=257)), ("max_distance_negative", dict(max_distance=-1)), ("max_du_nan", dict(max_du=NAN)),
        ("q_desc_misaligned", dict(q_desc=P + 8)), ("t_desc_misaligned", dict(t_desc=P + 4)), ("t_pos_misaligned", dict(t_pos=P + 4)),
        ("empty", {}), ("keys_null+nprob_negative", dict(keys=0, nprob=-1)), ("t_stride_0+max_distance_257", dict(t_stride=0, max_distance=257)),
        ("max_distance_257+max_du_nan", dict(max_distance=257, max_du=NAN)), ("max_du_nan+q_desc_misaligned", dict(max_du=NAN, q_desc=P + 8)),
        ("q_desc_misaligned+q_pos_misaligned", dict(q_desc=P + 8, q_pos=P + 4)), ("q_pos_misaligned", dict(q_pos=P + 4))]
    out.append(("sosvo_match_hamming_gated", gated, gated_ok, gated_cases + [("min_dv_nan", dict(min_dv=NAN))]))
    cyc = gated.replace("min_dv max_du", "max_du period")
    out.append(("sosvo_match_hamming_gated_cyclic", cyc, dict(gated_ok, period=1200.0), gated_cases + [
        ("period_half", dict(period=1200.5)), ("period_0", dict(period=0.0)), ("period_16385", dict(period=16385.0)), ("period_nan", dict(period=NAN)),
        ("max_du_nan+period_0", dict(max_du=NAN, period=0.0)), ("period_0+q_desc_misaligned", dict(period=0.0, q_desc=P + 8))]))
    ratio = gated.replace("max_distance keys", "max_distance ratio_64ths keys rivals")
    out.append(("sosvo_match_hamming_ratio", ratio, dict(gated_ok, ratio_64ths=48, rivals=P), [
        ("nq_null", dict(nq=0)), ("keys_null", dict(keys=0)), ("rivals_null", dict(rivals=0)), ("q_pos_alone", dict(t_pos=0)), ("t_pos_alone", dict(q_pos=0)),
        ("ratio_0", dict(ratio_64ths=0)), ("ratio_64", dict(ratio_64ths=64))] + sizes + [
        ("max_distance_257", dict(max_distance=257)), ("min_dv_nan", dict(min_dv=NAN)), ("max_du_nan", dict(max_du=NAN)),
        ("t_pos_misaligned", dict(t_pos=P + 4)), ("plain_max_distance_64", dict(q_pos=0, t_pos=0)),
        ("plain_empty", dict(q_pos=0, t_pos=0, max_distance=256)), ("plain_min_dv_nan", dict(q_pos=0, t_pos=0, max_distance=256, min_dv=NAN)),
        ("q_desc_misaligned", dict(q_desc=P + 8)), ("keys_misaligned", dict(keys=P + 2)), ("rivals_misaligned", dict(rivals=P + 1)), ("empty", {}),
        ("nq_null+rivals_null", dict(nq=0, rivals=0)), ("rivals_null+q_pos_alone", dict(rivals=0, t_pos=0)), ("q_pos_alone+ratio_0", dict(t_pos=0, ratio_64ths=0)),
        ("ratio_0+nprob_negative", dict(ratio_64ths=0, nprob=-1)), ("t_stride_0+max_distance_257", dict(t_stride=0, max_distance=257)),
        ("t_stride_0+plain_max_distance_64", dict(t_stride=0, q_pos=0, t_pos=0)), ("max_distance_257+max_du_nan", dict(max_distance=257, max_du=NAN)),
        ("max_du_nan+q_pos_misaligned", dict(max_du=NAN, q_pos=P + 4)), ("q_pos_misaligned+q_desc_misaligned", dict(q_pos=P + 4, q_desc=P + 8)),
        ("plain_max_distance_64+q_desc_misaligned", dict(q_pos=0, t_pos=0, q_desc=P + 8)), ("q_desc_misaligned+keys_misaligned", dict(q_desc=P + 8, keys=P + 2))]))

    frames = [("rows_0", dict(rows=0)), ("rows_16385", dict(rows=16385)), ("cols_0", dict(cols=0)), ("cols_16385", dict(cols=16385))]
    census = "gray nimg rows cols flags census_out"
    out.append(("sosvo_census_9x7", census, dict(gray=P, nimg=1, rows=3, cols=5, flags=0, census_out=P), [
        ("gray_null", dict(gray=0)), ("census_out_null", dict(census_out=0))] + frames + [
        ("nimg_0", dict(nimg=0)), ("nimg_65536", dict(nimg=65536)), ("flag_2", dict(flags=2)), ("flag_3", dict(flags=3)),
        ("gray_null+rows_0", dict(gray=0, rows=0)), ("rows_0+nimg_0", dict(rows=0, nimg=0)), ("nimg_0+flag_2", dict(nimg=0, flags=2))]))
    dense = "top bot n rows cols mask min_disparity P1 P2 uniqueness lr_max flags d16_out S_out"
    out.append(("sosvo_dense_stereo", dense, dict(top=P, bot=P, n=2, rows=3, cols=5, mask=0, min_disparity=0, P1=8, P2=32, uniqueness=10,
                                                  lr_max=1, flags=0, d16_out=P, S_out=0), [
        ("top_null", dict(top=0)), ("d16_out_null", dict(d16_out=0))] + frames + [
        ("n_0", dict(n=0)), ("n_32768", dict(n=32768)), ("P1_negative", dict(P1=-1)), ("P1_above_P2", dict(P1=33)), ("P2_8192", dict(P2=8192)),
        ("uniqueness_100", dict(uniqueness=100)), ("uniqueness_negative", dict(uniqueness=-1)), ("min_disparity_negative", dict(min_disparity=-1)),
        ("min_disparity_1025", dict(min_disparity=1025)), ("flag_2", dict(flags=2)),
        ("top_null+rows_0", dict(top=0, rows=0)), ("rows_0+n_0", dict(rows=0, n=0)), ("n_0+P1_negative", dict(n=0, P1=-1)),
        ("P1_negative+uniqueness_100", dict(P1=-1, uniqueness=100)), ("uniqueness_100+min_disparity_negative", dict(uniqueness=100, min_disparity=-1)),
        ("min_disparity_negative+flag_2", dict(min_disparity=-1, flags=2))]))
    tri = "rig d16 n rows cols min_d16 max_d16 X_out"
    out.append(("sosvo_dense_triangulate", tri, dict(rig=rig, d16=P, n=2, rows=3, cols=5, min_d16=0, max_d16=1024, X_out=P), [
        ("rig_null", dict(rig=0)), ("X_out_null", dict(X_out=0))] + frames + [
        ("n_0", dict(n=0)), ("n_32768", dict(n=32768)), ("panoramas_differ", dict(rig=rig_differs)),
        ("d16_null+rows_0", dict(d16=0, rows=0)), ("rows_0+n_0", dict(rows=0, n=0)), ("n_0+panoramas_differ", dict(n=0, rig=rig_differs))]))
    speckle = "d16 n rows cols max_size max_diff flags d16_out labels_out"
    out.append(("sosvo_dense_speckle", speckle, dict(d16=P, n=1, rows=9, cols=16, max_size=10, max_diff=16, flags=0, d16_out=P, labels_out=0), [
        ("d16_null", dict(d16=0)), ("d16_out_null", dict(d16_out=0))] + frames + [
        ("n_0", dict(n=0)), ("n_32768", dict(n=32768)), ("max_size_negative", dict(max_size=-1)), ("max_diff_negative", dict(max_diff=-1)),
        ("max_diff_32768", dict(max_diff=32768)), ("flag_2", dict(flags=2)),
        ("d16_null+rows_0", dict(d16=0, rows=0)), ("rows_0+n_0", dict(rows=0, n=0)), ("n_0+max_size_negative", dict(n=0, max_size=-1)),
        ("max_size_negative+max_diff_negative", dict(max_size=-1, max_diff=-1)), ("max_diff_negative+flag_2", dict(max_diff=-1, flags=2))]))
    return out


def record():
    """-> [[entry point, case, status, message]] from the library of this tree, on cuda:0."""
    import torch
    lib = _lib.load()
    buf = torch.zeros(512, dtype=torch.uint8, device="cuda:0")
    P = (buf.data_ptr() + 255) & ~255
    ctx = c_p()
    assert lib.sosvo_create(ctypes.byref(ctx), 0, None) == 0
    out, keep = [], []
    try:
        for entry, names, accepted, cases in table(P, keep):
            names = names.split()
            fn = getattr(lib, entry)
            if entry not in _lib.SIGNATURES:      # the internal ..._slots form: the public one's signature with the table after nframes
                public = list(_lib.SIGNATURES[entry[:-len("_slots")]][1])
                fn.restype, fn.argtypes = c_i32, public[:11] + [c_p] + public[11:]
            assert len(fn.argtypes) == 1 + len(names), entry
            assert len(set(c for c, _ in cases)) == len(cases), entry
            for case, wrong in cases:
                assert set(wrong) <= set(names), (entry, case)
                status = fn(ctx, *[dict(accepted, **wrong)[n] for n in names])
                message = lib.sosvo_last_error(ctx).decode() if status != 0 else ""
                out.append([entry, case, status, message])
        torch.cuda.synchronize()
    finally:
        lib.sosvo_destroy(ctx)
    return out


def main(argv):
    if len(argv) != 2:
        sys.exit(__doc__)
    out = record()
    with open(argv[1], "w") as f:      # one case per line
        f.write("[\n" + ",\n".join(json.dumps(o) for o in out) + "\n]\n")
    print("%d cases of %d entry points, %d distinct messages -> %s" % (len(out), len(set(o[0] for o in out)), len(set((o[0], o[3]) for o in out)), argv[1]))


if __name__ == "__main__":
    main(sys.argv)
