// sosvo_frame_pair_batch -- the whole hot path for B independent frame pairs behind ONE C-ABI call:
// the order of operations of OmniStereoModel.set_current_omni_image + StereoPanoramicFrame.__init__
// (omnistereo/camera_models.py:3107-3120, pose_est_tools.py:271-402) for both frames of every pair, then
// TrackerStereoSE3.track_frame (pose_est_tools.py:736-847) per pair.  It only sequences the stage entry points
// of this library on the context's stream (no host synchronisation, no allocation: every intermediate lives in
// the caller's workspace), so its results are those of calling the stages one by one.
#include <vector>

#include "common.h"

namespace {

// the ORB detector's extra buffers (sosvo_detect_describe_orb): oriented keypoints, responses, the mask pyramid.  Carved
// after everything else, and only for ORB, so that the other detectors' workspaces keep their sizes and layout.
struct OrbBufs {
  float *kp4 = nullptr, *resp = nullptr;
  uint32_t* mask_pyr = nullptr;
};
OrbBufs carve_orb(Carver& cv, int detector, size_t P, size_t cap, size_t nsets, int rows, int cols) {
  OrbBufs o;
  if (detector != SOSVO_DETECTOR_ORB) return o;
  o.kp4 = cv.take<float>(P * cap * 4);
  o.resp = cv.take<float>(P * cap);
  o.mask_pyr = cv.take<uint32_t>(nsets * (size_t)sosvo_orb_pyramid_pixels(rows, cols));
  return o;
}

// a detector the batch entry points run, with a capacity its stages accept (sosvo_detect_describe_orb: cap <= 2048)
bool detector_ok(int detector, int kp_cap) {
  if (detector == SOSVO_DETECTOR_ORB) return kp_cap <= 2048;
  return detector == SOSVO_DETECTOR_GFT || detector == SOSVO_DETECTOR_FAST || detector == SOSVO_DETECTOR_AGAST;
}
int rgbd_detector(const sosvo_rgbd_batch_cfg& c) { return SOSVO_RGBD_DETECTOR_OF(c.flags); }

// ---- mutual-consistency matching (SOSVO_FLAG_CROSS_CHECK_*, camera_models.py:401) -------------------------------------
// A matching step of n problems over ONE descriptor store runs as 2 n problems of one sosvo_match_hamming launch: problem
// p < n is the forward search (query block q[p], train block t[p]), problem n + p the same search with the roles swapped.
// The slot tables hold both halves: q_slot = [q | t], t_slot = [t | q], 2 n entries each, and the keys [2 n, stride] are
// forward rows first.  Carved only when the switch is set, after everything else, so that the other members keep their
// offsets and the workspace its size.
struct MutualTabs {
  int32_t *q_slot = nullptr, *t_slot = nullptr;
};
MutualTabs carve_mutual(Carver& cv, bool on, size_t n) {
  MutualTabs m;
  if (!on) return m;
  m.q_slot = cv.take<int32_t>(2 * n);
  m.t_slot = cv.take<int32_t>(2 * n);
  return m;
}
bool cross_stereo(const sosvo_batch_cfg& c) { return (c.ransac_flags & SOSVO_FLAG_CROSS_CHECK_STEREO) != 0; }
bool cross_f2f(const sosvo_batch_cfg& c) { return (c.ransac_flags & SOSVO_FLAG_CROSS_CHECK_F2F) != 0; }
bool cross_f2f(const sosvo_rgbd_batch_cfg& c) { return (c.flags & SOSVO_FLAG_CROSS_CHECK_F2F) != 0; }
// (an RGB-D camera has no static stereo to cross-check)
// ---- the ratio rule (SOSVO_FLAG_RATIO_*, sosvo_match_hamming_ratio): a matching step with its switch set runs the fused
// ratio form of its search, plain or under the step's Gate.  r64 = 0: off, the step is the call it always was.  `rivals` is
// the step's runner-up / split-merge buffer, as large as the step's keys; carved only when a switch is set, after everything
// else, so that the other members keep their offsets and the workspace its size.
struct Ratio {
  int32_t r64 = 0;
  uint32_t* rivals = nullptr;
};
// a switch bit needs a ratio; the field alone is ignored
bool ratio_flags_ok(int32_t flags) {
  return (flags & (SOSVO_FLAG_RATIO_STEREO | SOSVO_FLAG_RATIO_F2F)) == 0 || SOSVO_RATIO_64THS_OF(flags) != 0;
}
int32_t ratio_of(int32_t flags, int32_t bit) { return (flags & bit) ? SOSVO_RATIO_64THS_OF(flags) : 0; }
int32_t ratio_stereo(const sosvo_batch_cfg& c) { return ratio_of(c.ransac_flags, SOSVO_FLAG_RATIO_STEREO); }
int32_t ratio_f2f(const sosvo_batch_cfg& c) { return ratio_of(c.ransac_flags, SOSVO_FLAG_RATIO_F2F); }
int32_t ratio_f2f(const sosvo_rgbd_batch_cfg& c) { return ratio_of(c.flags, SOSVO_FLAG_RATIO_F2F); }
Ratio carve_ratio(Carver& cv, int32_t r64, size_t n_keys) {
  Ratio r;
  if (!r64) return r;
  r.r64 = r64;
  r.rivals = cv.take<uint32_t>(n_keys);
  return r;
}
constexpr const char* kBadRatioFlags = "SOSVO_FLAG_RATIO_STEREO / _F2F need SOSVO_RATIO_64THS(r), r in 1..63";

// ---- Lucas-Kanade tracking (SOSVO_FLAG_LK_F2F): the tracking step follows the reference frame's points into the current
// frame's images instead of matching descriptors.  The options of the matcher it replaces are refused with it.
bool lk_f2f(const sosvo_batch_cfg& c) { return (c.ransac_flags & SOSVO_FLAG_LK_F2F) != 0; }
bool lk_flags_ok(int32_t flags) {
  return (flags & SOSVO_FLAG_LK_F2F) == 0 ||
         (flags & (SOSVO_FLAG_CROSS_CHECK_F2F | SOSVO_FLAG_GATED_F2F | SOSVO_FLAG_RATIO_F2F)) == 0;
}
constexpr const char* kBadLkFlags =
    "SOSVO_FLAG_LK_F2F replaces the frame-to-frame matcher: SOSVO_FLAG_CROSS_CHECK_F2F / _GATED_F2F / _RATIO_F2F cannot be set with it";
// ---- sub-pixel static stereo (SOSVO_FLAG_LK_STEREO): sosvo_refine_stereo_lk between the sort and the stereo assemble, with the
// context's settings.  Its status flags are carved only when the switch is set, after everything else.
bool lk_stereo(const sosvo_batch_cfg& c) { return (c.ransac_flags & SOSVO_FLAG_LK_STEREO) != 0; }
// ---- cyclic panorama columns (SOSVO_FLAG_CYCLIC_F2F): the frame-to-frame |du| gate is cyclic in the
// assemble and, under SOSVO_FLAG_GATED_F2F, inside the matcher; under SOSVO_FLAG_LK_F2F the store's pyramids and the tracker
// are cyclic too, which needs every level the store may hold to be one period (cols % 2^(SOSVO_LK_MAX_LEVELS - 1) == 0: the
// workspace functions take no context).  The ratio form of the gated matcher has no cyclic instantiation.
bool cyclic_f2f(const sosvo_batch_cfg& c) { return (c.ransac_flags & SOSVO_FLAG_CYCLIC_F2F) != 0; }
constexpr const char* kBadCyclicCols = "SOSVO_FLAG_CYCLIC_F2F with SOSVO_FLAG_LK_F2F needs cols % 8 == 0 (every level of the store is one period)";
constexpr const char* kBadCyclicRatio =
    "SOSVO_FLAG_CYCLIC_F2F: the ratio form of the gated frame-to-frame matcher (SOSVO_FLAG_GATED_F2F | SOSVO_FLAG_RATIO_F2F) has no cyclic gate";
// ---- the seam-free front end (SOSVO_FLAG_SEAM_FREE): the image stages run on panoramas padded by
// SOSVO_SEAM_HALO cyclic columns on either side (the caller's table and mask bits are the padded ones), the keypoints are
// unpadded before the stereo assemble.  c.cols stays the period; run_cols is what the image stages see.
bool seam_free(const sosvo_batch_cfg& c) { return (c.ransac_flags & SOSVO_FLAG_SEAM_FREE) != 0; }
int run_cols(const sosvo_batch_cfg& c) { return seam_free(c) ? c.cols + 2 * SOSVO_SEAM_HALO : c.cols; }
constexpr int kSeamReach = 35;  // columns a stage may read around a keypoint of the original columns
const char* seam_free_msg(const sosvo_batch_cfg& c) {
  if (!seam_free(c)) return nullptr;
  if (!cyclic_f2f(c)) return "SOSVO_FLAG_SEAM_FREE needs SOSVO_FLAG_CYCLIC_F2F";
  if (c.detector == SOSVO_DETECTOR_ORB) return "SOSVO_FLAG_SEAM_FREE: the ORB detector's pyramid levels keep borders the halo does not cover";
  if (c.edge > 31) return "SOSVO_FLAG_SEAM_FREE needs edge <= 31";
  if (c.cols < SOSVO_SEAM_HALO || c.cols + 2 * SOSVO_SEAM_HALO > 16384) return "SOSVO_FLAG_SEAM_FREE needs 40 <= cols and cols + 80 <= 16384";
  return nullptr;
}
// (at call time: the settings live in the context) the stereo-LK windows stay inside the halo's clean columns
bool seam_free_stereo_lk_ok(const sosvo_batch_cfg& c, const sosvo_stereo_lk_options& o) {
  if (!seam_free(c) || !lk_stereo(c)) return true;
  const double shift = o.max_shift > 0.0 ? o.max_shift : (double)o.half;
  return 2.0 + o.half + ceil(shift) <= (double)kSeamReach;
}
constexpr const char* kBadSeamStereoLk = "SOSVO_FLAG_SEAM_FREE with SOSVO_FLAG_LK_STEREO needs 2 + half + ceil(max_shift) <= 35";
// what every omni entry point asks of cfg->ransac_flags and the shape (nullptr: fine)
const char* omni_flags_msg(const sosvo_batch_cfg& c) {
  const int32_t flags = c.ransac_flags;
  if (seam_free_msg(c)) return seam_free_msg(c);
  if (!ratio_flags_ok(flags)) return kBadRatioFlags;
  if (!lk_flags_ok(flags)) return kBadLkFlags;
  if (cyclic_f2f(c) && lk_f2f(c) && c.cols % (1 << (SOSVO_LK_MAX_LEVELS - 1)) != 0) return kBadCyclicCols;
  if (cyclic_f2f(c) && (flags & SOSVO_FLAG_GATED_F2F) && (flags & SOSVO_FLAG_RATIO_F2F)) return kBadCyclicRatio;
  return nullptr;
}
// the gray rows the front end computes are those of sosvo_gray_rows_needed (GFT with the fused median), else all rows
bool gray_rows_known(const sosvo_batch_cfg& c) {
  return c.detector == SOSVO_DETECTOR_GFT && (c.median_ksize == 3 || c.median_ksize == 5 || c.median_ksize == 11);
}

// (SOSVO_FLAG_SUBPIX is refused with them: the RGB-D assemble stage reads depth at the keypoints' integer pixels)
bool rgbd_stereo_flags_ok(const sosvo_rgbd_batch_cfg& c) {
  return (c.flags & (SOSVO_FLAG_CROSS_CHECK_STEREO | SOSVO_FLAG_GATED_STEREO | SOSVO_FLAG_RATIO_STEREO | SOSVO_FLAG_SUBPIX |
                     SOSVO_FLAG_LK_F2F)) == 0;
}
constexpr const char* kRgbdStereoFlags =
    "SOSVO_FLAG_CROSS_CHECK_STEREO / SOSVO_FLAG_GATED_STEREO / SOSVO_FLAG_RATIO_STEREO: an RGB-D camera has no static stereo; "
    "SOSVO_FLAG_SUBPIX: depth is read at integer pixels; SOSVO_FLAG_LK_F2F: the omni family's";
bool rgbd_flags_ok(const sosvo_rgbd_batch_cfg& c) { return rgbd_stereo_flags_ok(c) && ratio_flags_ok(c.flags); }

// ---- gated matching (SOSVO_FLAG_GATED_*): the 1-NN search among the trains that pass the assemble stage's own pixel gate.
// A Gate holds that stage's arguments; with `on` clear a matching step is the plain sosvo_match_hamming call it always was.
struct Gate {
  bool on;
  double min_dv, max_du;
  int32_t max_distance;
  double period = 0.0;  // > 0: the u side is cyclic with this period (sosvo_match_hamming_gated_cyclic; no v side, no ratio form)
};
int32_t gate_cap(int32_t flags) { return SOSVO_GATED_MAX_DIST_OF(flags) ? SOSVO_GATED_MAX_DIST_OF(flags) : 256; }
Gate gate_stereo(const sosvo_batch_cfg& c, const sosvo_rig& rig) {  // stereo_assemble_frame's sv_pixel_gate
  return Gate{(c.ransac_flags & SOSVO_FLAG_GATED_STEREO) != 0, rig.stereo_min_disp, rig.stereo_max_hdiff, gate_cap(c.ransac_flags)};
}
Gate gate_f2f(const sosvo_batch_cfg& c, const sosvo_rig& rig) {  // f2f_assemble_kernel's: |du| only; off for f2f_max_hdiff <= 0 (< 0: gate skipped, 0: sv_pixel_gate passes all)
  return Gate{(c.ransac_flags & SOSVO_FLAG_GATED_F2F) != 0, -1.0, rig.f2f_max_hdiff, gate_cap(c.ransac_flags)};
}
Gate gate_f2f(const sosvo_rgbd_batch_cfg& c) {  // f2f_assemble_central_kernel's
  return Gate{(c.flags & SOSVO_FLAG_GATED_F2F) != 0, -1.0, c.f2f_max_hdiff, gate_cap(c.flags)};
}

// q == nullptr: static stereo, bucket p's query block is n + p (bottom view), its train block p (top view);
// otherwise the slot pairs of a tracking call: query = current frame, train = reference frame
__global__ void mutual_tabs_kernel(int n, const int32_t* __restrict__ q, const int32_t* __restrict__ t,
                                   int32_t* __restrict__ q_slot, int32_t* __restrict__ t_slot) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int qs = q ? q[p] : n + p, ts = q ? t[p] : p;
  q_slot[p] = qs;
  t_slot[p] = ts;
  q_slot[n + p] = ts;
  t_slot[n + p] = qs;
}

// ---- the workspace of the omni family: front-end temporaries of one WINDOW of frames, a frame STORE of `slots` frame
// records, tracking of up to cfg.n_pairs slot pairs per call.  The structs below are what the runners take; each is carved
// member by member, so a buffer has one name from the carve to its use.
struct FrontEndTmp {
  uint8_t *pano, *gray, *desc;
  float* kp;
  int32_t *n, *status, *s_order, *n_cand, *gray_rows;
  uint32_t* s_keys;
  uint8_t* lk_status;  // (nullptr without SOSVO_FLAG_LK_STEREO)
  OrbBufs orb;
  MutualTabs mutual;
  Ratio ratio;
};
FrontEndTmp carve_front_end(Carver& cv, const sosvo_batch_cfg& c, size_t F) {
  FrontEndTmp t{};
  const size_t NI = 2 * F, P = NI * c.nmask, cap = c.kp_cap, npx = (size_t)c.rows * run_cols(c);
  const bool fused = c.median_ksize <= 1 || c.median_ksize == 3 || c.median_ksize == 5 || c.median_ksize == 11;  // K1 inside the median / gray kernel
  t.pano = fused ? nullptr : cv.take<uint8_t>(NI * npx * 3);
  t.gray = cv.take<uint8_t>(NI * npx);
  t.kp = cv.take<float>(P * cap * 2);
  t.n = cv.take<int32_t>(P);
  t.status = cv.take<int32_t>(P);
  t.desc = cv.take<uint8_t>(P * cap * 32);
  t.s_keys = cv.take<uint32_t>((cross_stereo(c) ? P : P / 2) * cap);  // (cross-check: the reverse keys follow the forward ones)
  t.s_order = cv.take<int32_t>(P / 2 * cap);
  t.n_cand = cv.take<int32_t>(F);
  t.gray_rows = cv.take<int32_t>(4);
  return t;
}

// PanoramicCorrespondences as SoA, slot-major
struct FrameStore {
  float *m_top, *m_bot;
  uint8_t *d_top, *d_bot;
  double *X, *b_top, *b_bot;
  int32_t* M;
  FrameStore at(size_t slot, size_t Fc) const {  // the records from `slot` on
    const size_t o = slot * Fc;
    FrameStore v = *this;
    v.m_top += 2 * o;
    v.m_bot += 2 * o;
    v.d_top += 32 * o;
    v.d_bot += 32 * o;
    v.X += 3 * o;
    v.b_top += 3 * o;
    v.b_bot += 3 * o;
    v.M += slot;
    return v;
  }
};
FrameStore carve_store(Carver& cv, size_t S, size_t Fc) {
  FrameStore s{};
  s.m_top = cv.take<float>(S * Fc * 2);
  s.m_bot = cv.take<float>(S * Fc * 2);
  s.d_top = cv.take<uint8_t>(S * Fc * 32);
  s.d_bot = cv.take<uint8_t>(S * Fc * 32);
  s.X = cv.take<double>(S * Fc * 3);
  s.b_top = cv.take<double>(S * Fc * 3);
  s.b_bot = cv.take<double>(S * Fc * 3);
  s.M = cv.take<int32_t>(S);
  return s;
}

// The tracker's temporaries (SOSVO_FLAG_LK_F2F), [2 B, ...]: problem v * B + i is view v of pair i.  from / to: its images in
// the store, n: its point count M[ref[i]], pt: where its points begin in m_top (in points; the bottom view's lie in m_bot).
// Carved only when the switch is set, after everything else.
struct LkTmp {
  float *next = nullptr, *err = nullptr, *back = nullptr;
  uint8_t* status = nullptr;
  int32_t *from = nullptr, *to = nullptr, *n = nullptr;
  int64_t* pt = nullptr;
};
LkTmp carve_lk_tmp(Carver& cv, bool on, size_t B, size_t Fc) {
  LkTmp t;
  if (!on) return t;
  t.next = cv.take<float>(2 * B * Fc * 2);
  t.status = cv.take<uint8_t>(2 * B * Fc);
  t.err = cv.take<float>(2 * B * Fc);
  t.back = cv.take<float>(2 * B * Fc * 2);
  t.from = cv.take<int32_t>(2 * B);
  t.to = cv.take<int32_t>(2 * B);
  t.n = cv.take<int32_t>(2 * B);
  t.pt = cv.take<int64_t>(2 * B);
  return t;
}
// The store's images (SOSVO_FLAG_LK_F2F; sosvo_lk_images, common.h): every level [2 * slots, rows_l, cols_l], each 256-byte
// aligned.  level0 != nullptr (a pair batch: frame i in slot i of 2 * n_pairs): the front end's gray buffer is level 0.
// `on` clear: level[0] stays null, which is how the runners see the switch.
sosvo_lk_images carve_lk_images(Carver& cv, bool on, size_t S, int rows, int cols, uint8_t* level0, bool in_place) {
  sosvo_lk_images im{};
  if (!on) return im;
  im.slots = (int32_t)S;
  im.rows = rows;
  im.cols = cols;
  for (int l = 0; l < SOSVO_LK_MAX_LEVELS; ++l) {
    im.level[l] = l == 0 && in_place ? level0 : cv.take<uint8_t>(2 * S * (size_t)rows * cols);
    rows = (rows + 1) / 2;
    cols = (cols + 1) / 2;
  }
  return im;
}

struct TrackTmp {
  int32_t *ref_frame, *cur_frame, *o_top, *o_bot, *cam, *cq, *ct, *cn, *cn_top, *idx, *n_inl, *info, *lm_iters;
  uint32_t *k_top, *k_bot;
  uint8_t* mask;
  double *f, *p, *T_ransac, *T, *cam_off, *cam_rot, *lm_cost;
  MutualTabs mutual;
  Ratio ratio;  // (one buffer serves both views: their matching steps follow each other on the stream)
  LkTmp lk;
};
TrackTmp carve_track(Carver& cv, size_t B, size_t Fc, bool mutual) {
  TrackTmp t{};
  const size_t Cc = 2 * Fc, Kr = mutual ? 2 : 1;  // (cross-check: the reverse keys follow the forward ones)
  t.ref_frame = cv.take<int32_t>(B);
  t.cur_frame = cv.take<int32_t>(B);
  t.k_top = cv.take<uint32_t>(Kr * B * Fc);
  t.k_bot = cv.take<uint32_t>(Kr * B * Fc);
  t.o_top = cv.take<int32_t>(B * Fc);
  t.o_bot = cv.take<int32_t>(B * Fc);
  t.f = cv.take<double>(B * Cc * 3);
  t.p = cv.take<double>(B * Cc * 3);
  t.cam = cv.take<int32_t>(B * Cc);
  t.cq = cv.take<int32_t>(B * Cc);
  t.ct = cv.take<int32_t>(B * Cc);
  t.cn = cv.take<int32_t>(B);
  t.cn_top = cv.take<int32_t>(B);
  t.T_ransac = cv.take<double>(B * 12);
  t.mask = cv.take<uint8_t>(B * Cc);
  t.idx = cv.take<int32_t>(B * Cc);
  t.n_inl = cv.take<int32_t>(B);
  t.info = cv.take<int32_t>(B * 4);
  t.T = cv.take<double>(B * 12);
  t.cam_off = cv.take<double>(2 * 3);
  t.cam_rot = cv.take<double>(2 * 9);
  t.lm_cost = cv.take<double>(B);
  t.lm_iters = cv.take<int32_t>(B);
  return t;
}

struct Workspace {
  FrontEndTmp fe;
  FrameStore store;
  TrackTmp tt;
  sosvo_lk_images img;      // (level[0] == nullptr without SOSVO_FLAG_LK_F2F)
  bool img_in_place;        // level 0 is fe.gray: nothing to copy
  const int32_t* img_rows;  // the row range of the images: fe.gray_rows where the front end computes only those, else nullptr
  size_t bytes;
};
// (a pair batch is the sequence layout with window = slots = 2 * n_pairs; base == nullptr: sizes only)
Workspace carve(const sosvo_batch_cfg& c, size_t window, size_t slots, void* base, bool pair_batch = false) {
  Carver cv{reinterpret_cast<char*>(base)};
  Workspace ws;
  ws.fe = carve_front_end(cv, c, window);
  ws.store = carve_store(cv, slots, c.frame_cap);
  ws.tt = carve_track(cv, c.n_pairs, c.frame_cap, cross_f2f(c));
  ws.fe.orb = carve_orb(cv, c.detector, 2 * window * c.nmask, c.kp_cap, 2, c.rows, c.cols);  // (never with SOSVO_FLAG_SEAM_FREE)
  ws.fe.mutual = carve_mutual(cv, cross_stereo(c), window * c.nmask);
  ws.tt.mutual = carve_mutual(cv, cross_f2f(c), c.n_pairs);
  ws.fe.ratio = carve_ratio(cv, ratio_stereo(c), (cross_stereo(c) ? 2 : 1) * window * c.nmask * c.kp_cap);
  ws.tt.ratio = carve_ratio(cv, ratio_f2f(c), (cross_f2f(c) ? 2 : 1) * (size_t)c.n_pairs * c.frame_cap);
  // (SOSVO_FLAG_SEAM_FREE: the front end's rows are padded, level 0 is their interior crop and has a buffer of its own)
  ws.img_in_place = pair_batch && !seam_free(c);
  ws.img = carve_lk_images(cv, lk_f2f(c), slots, c.rows, c.cols, ws.fe.gray, ws.img_in_place);
  ws.img_rows = gray_rows_known(c) ? ws.fe.gray_rows : nullptr;
  ws.tt.lk = carve_lk_tmp(cv, lk_f2f(c), c.n_pairs, c.frame_cap);
  ws.fe.lk_status = lk_stereo(c) ? cv.take<uint8_t>(window * c.nmask * (size_t)c.kp_cap) : nullptr;
  ws.bytes = cv.off;
  return ws;
}

struct Foci {
  double top[3], bot[3];
};
Foci foci_of(const sosvo_rig* rig) {
  Foci foci;
  for (int k = 0; k < 3; ++k) {
    foci.top[k] = rig->F_top[k];
    foci.bot[k] = rig->F_bot[k];
  }
  return foci;
}

// pair i tracks frame 2i + 1 against frame 2i; the two mirrors' foci are the non-central rig (identity rotations)
__global__ void batch_setup_kernel(int npairs, Foci foci, int32_t* __restrict__ ref_frame, int32_t* __restrict__ cur_frame,
                                   double* __restrict__ cam_off, double* __restrict__ cam_rot) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < npairs) {
    ref_frame[i] = 2 * i;
    cur_frame[i] = 2 * i + 1;
  }
  if (i < 3) {
    cam_off[i] = foci.top[i];
    cam_off[3 + i] = foci.bot[i];
  }
  if (i < 18) cam_rot[i] = (i % 9) % 4 == 0 ? 1.0 : 0.0;
}

// [B,16]: refined 3x4 pose, n_inliers, n_correspondences, status, RANSAC best iteration
__global__ void batch_results_kernel(int npairs, const double* __restrict__ T, const int32_t* __restrict__ n_inl,
                                     const int32_t* __restrict__ n_corr, const int32_t* __restrict__ info,
                                     double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npairs) return;
  for (int k = 0; k < 12; ++k) out[16 * i + k] = T[12 * i + k];
  out[16 * i + 12] = (double)n_inl[i];
  out[16 * i + 13] = (double)n_corr[i];
  out[16 * i + 14] = (double)info[4 * i + 2];
  out[16 * i + 15] = (double)info[4 * i + 0];
}


// ---- sequence mode: the front end over a WINDOW of frames writes into the store, slot pairs of the store are tracked ----
constexpr int kSeqArgPairs = 16;  // slot pairs that travel as kernel arguments (no host-to-device copy per call)
struct SlotPairs {
  int32_t ref[kSeqArgPairs], cur[kSeqArgPairs];
};
// ... and their seeds (the ..._track_seeds entry points; seeds_out == nullptr: the call has one scalar seed)
struct PairSeeds {
  uint64_t seed[kSeqArgPairs];
};
// (cam_off == nullptr: the RGB-D family, a central camera with nothing but the slot pairs and seeds to set up)
__global__ void seq_setup_kernel(int npairs, SlotPairs sp, PairSeeds ps, Foci foci, int32_t* __restrict__ ref_frame,
                                 int32_t* __restrict__ cur_frame, uint64_t* __restrict__ seeds_out, double* __restrict__ cam_off,
                                 double* __restrict__ cam_rot) {
  const int i = threadIdx.x;
  if (i < npairs && i < kSeqArgPairs) {
    ref_frame[i] = sp.ref[i];
    cur_frame[i] = sp.cur[i];
    if (seeds_out) seeds_out[i] = ps.seed[i];
  }
  if (!cam_off) return;
  if (i < 3) {
    cam_off[i] = foci.top[i];
    cam_off[3 + i] = foci.bot[i];
  }
  if (i < 18) cam_rot[i] = (i % 9) % 4 == 0 ? 1.0 : 0.0;
}

// A frame store of either family as the copy kernel sees it: per field of a record the base pointer and the bytes of one
// entry (8 for m*, 32 for d*, 24 for X and b*: all multiples of 8, and every base is 256-byte aligned), then the counts.
// Unused fields have 0 bytes.
constexpr int kStoreFields = 7;
struct StoreFields {
  char* base[kStoreFields];
  int32_t bytes[kStoreFields];
  int32_t* M;
};

// Frame records of the store -> other slots (a frame promoted to keyframe outlives its window), k (source, destination)
// pairs in one launch: workgroup (j, c) copies every gridDim.y-th block of 256 8-byte words of each field of pair j (the
// entries of a slot are contiguous within a field).  The host has checked that no slot is written twice or read and written.
struct CopyPairs {
  int32_t src[kSeqArgPairs], dst[kSeqArgPairs];
};
constexpr int kCopyChunks = 4;
__global__ __launch_bounds__(256) void seq_copy_slots_kernel(CopyPairs cp, const int32_t* __restrict__ src_list,
                                                             const int32_t* __restrict__ dst_list, int Fc, StoreFields st) {
  const int j = blockIdx.x;
  const int src = src_list ? src_list[j] : cp.src[j], dst = src_list ? dst_list[j] : cp.dst[j];
  const int n = min(st.M[src], Fc);
#pragma unroll
  for (int f = 0; f < kStoreFields; ++f) {
    const size_t slot_bytes = (size_t)Fc * st.bytes[f];
    const uint2* s = reinterpret_cast<const uint2*>(st.base[f] + src * slot_bytes);
    uint2* d = reinterpret_cast<uint2*>(st.base[f] + dst * slot_bytes);
    const int words = n * (st.bytes[f] / 8);
    for (int i = blockIdx.y * blockDim.x + threadIdx.x; i < words; i += gridDim.y * blockDim.x) d[i] = s[i];
  }
  if (blockIdx.y == 0 && threadIdx.x == 0) st.M[dst] = st.M[src];  // (no slot of the list is both read and written)
}

// ... and the images of those slots (SOSVO_FLAG_LK_F2F), in a launch of their own: workgroup (j, c, 2 l + v) copies every
// gridDim.y-th block of view v, level l of pair j -- whole images, also the rows outside the range, which nobody reads.
constexpr int kCopyImageChunks = 16;
__global__ __launch_bounds__(256) void seq_copy_images_kernel(CopyPairs cp, const int32_t* __restrict__ src_list,
                                                              const int32_t* __restrict__ dst_list, sosvo_lk_images im) {
  const int j = blockIdx.x, v = blockIdx.z & 1, l = blockIdx.z >> 1;
  const int src = src_list ? src_list[j] : cp.src[j], dst = src_list ? dst_list[j] : cp.dst[j];
  int rows = im.rows, cols = im.cols;
  for (int k = 0; k < l; ++k) {
    rows = (rows + 1) / 2;
    cols = (cols + 1) / 2;
  }
  const size_t npx = (size_t)rows * cols;
  sosvo_copy_bytes(im.level[l] + ((size_t)v * im.slots + dst) * npx, im.level[l] + ((size_t)v * im.slots + src) * npx, npx,
                   blockIdx.y * blockDim.x + threadIdx.x, gridDim.y * blockDim.x);
}

// The tracker's problems of B slot pairs (LkTmp): view v of pair i tracks the points of slot ref[i] from image
// v * slots + ref[i] to image v * slots + cur[i].  bot_pt: where m_bot begins, in points from m_top.
__global__ void lk_setup_kernel(int B, int slots, int Fc, const int32_t* __restrict__ ref, const int32_t* __restrict__ cur,
                                const int32_t* __restrict__ M, int64_t bot_pt, int32_t* __restrict__ from, int32_t* __restrict__ to,
                                int32_t* __restrict__ n, int64_t* __restrict__ pt) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= 2 * B) return;
  const int v = p / B, i = p - v * B;
  const int r = clampi(ref[i], 0, slots - 1), c = clampi(cur[i], 0, slots - 1);  // (the host has checked them)
  from[p] = v * slots + r;
  to[p] = v * slots + c;
  n[p] = M[r];
  pt[p] = v * bot_pt + (int64_t)r * Fc;
}

// ---- RGB-D variant (BASELINE config 5): the same three parts; a store of `slots` RGBDFrame records (keypoints with valid
// depth, descriptors, points, bearings)
struct RgbdFrontTmp {
  uint8_t *gray, *desc;
  float* kp;
  int32_t *n, *status;
  OrbBufs orb;
};
RgbdFrontTmp carve_rgbd_front_end(Carver& cv, const sosvo_rgbd_batch_cfg& c, size_t F) {
  RgbdFrontTmp t{};
  const size_t cap = c.kp_cap;
  t.gray = cv.take<uint8_t>(F * ((size_t)c.rows * c.cols));
  t.kp = cv.take<float>(F * cap * 2);
  t.n = cv.take<int32_t>(F);
  t.status = cv.take<int32_t>(F);
  t.desc = cv.take<uint8_t>(F * cap * 32);
  return t;
}

struct RgbdStore {
  float* m;
  uint8_t* d;
  double *X, *b;
  int32_t* M;
  RgbdStore at(size_t slot, size_t Fc) const {  // the records from `slot` on
    const size_t o = slot * Fc;
    RgbdStore v = *this;
    v.m += 2 * o;
    v.d += 32 * o;
    v.X += 3 * o;
    v.b += 3 * o;
    v.M += slot;
    return v;
  }
};
RgbdStore carve_rgbd_store(Carver& cv, size_t S, size_t Fc) {
  RgbdStore s{};
  s.m = cv.take<float>(S * Fc * 2);
  s.d = cv.take<uint8_t>(S * Fc * 32);
  s.X = cv.take<double>(S * Fc * 3);
  s.b = cv.take<double>(S * Fc * 3);
  s.M = cv.take<int32_t>(S);
  return s;
}

struct RgbdTrackTmp {
  int32_t *ref_frame, *cur_frame, *order, *cq, *ct, *cn, *idx, *n_inl, *info, *lm_iters;
  uint32_t* keys;
  uint8_t* mask;
  double *f, *p, *T_ransac, *T, *lm_cost;
  double *cam_off, *cam_rot;  // (never carved: a central camera has none, they stay null for the setup kernel)
  MutualTabs mutual;
  Ratio ratio;
};
RgbdTrackTmp carve_rgbd_track(Carver& cv, size_t B, size_t Fc, bool mutual) {
  RgbdTrackTmp t{};
  t.ref_frame = cv.take<int32_t>(B);
  t.cur_frame = cv.take<int32_t>(B);
  t.keys = cv.take<uint32_t>((mutual ? 2 : 1) * B * Fc);  // (cross-check: the reverse keys follow the forward ones)
  t.order = cv.take<int32_t>(B * Fc);
  t.f = cv.take<double>(B * Fc * 3);
  t.p = cv.take<double>(B * Fc * 3);
  t.cq = cv.take<int32_t>(B * Fc);
  t.ct = cv.take<int32_t>(B * Fc);
  t.cn = cv.take<int32_t>(B);
  t.T_ransac = cv.take<double>(B * 12);
  t.mask = cv.take<uint8_t>(B * Fc);
  t.idx = cv.take<int32_t>(B * Fc);
  t.n_inl = cv.take<int32_t>(B);
  t.info = cv.take<int32_t>(B * 4);
  t.T = cv.take<double>(B * 12);
  t.lm_cost = cv.take<double>(B);
  t.lm_iters = cv.take<int32_t>(B);
  return t;
}

struct RgbdWorkspace {
  RgbdFrontTmp fe;
  RgbdStore store;
  RgbdTrackTmp tt;
  size_t bytes;
};
RgbdWorkspace carve_rgbd(const sosvo_rgbd_batch_cfg& c, size_t window, size_t slots, void* base) {
  Carver cv{reinterpret_cast<char*>(base)};
  RgbdWorkspace ws;
  ws.fe = carve_rgbd_front_end(cv, c, window);
  ws.store = carve_rgbd_store(cv, slots, c.frame_cap);
  ws.tt = carve_rgbd_track(cv, c.n_pairs, c.frame_cap, cross_f2f(c));
  ws.fe.orb = carve_orb(cv, rgbd_detector(c), window, c.kp_cap, 1, c.rows, c.cols);
  ws.tt.mutual = carve_mutual(cv, cross_f2f(c), c.n_pairs);
  ws.tt.ratio = carve_ratio(cv, ratio_f2f(c), (cross_f2f(c) ? 2 : 1) * (size_t)c.n_pairs * c.frame_cap);
  ws.bytes = cv.off;
  return ws;
}

__global__ void pair_index_kernel(int npairs, int32_t* __restrict__ ref_frame, int32_t* __restrict__ cur_frame) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < npairs) {
    ref_frame[i] = 2 * i;
    cur_frame[i] = 2 * i + 1;
  }
}

// SOSVO_REQUIRE for a helper of the entry points: the error names the entry point `fn`, not the helper
#define REQUIRE_FOR(ctx, fn, cond, msg)                                \
  do {                                                                 \
    if (!(cond)) return sosvo_fail((ctx), SOSVO_ERR_ARG, (fn), msg);   \
  } while (0)

// Where the device keeps the seeds of a ..._track_seeds call: the slice of the LM costs.  8 bytes per pair both, and the
// costs are not written before the refinement, which runs after the last reader of the seeds (the hypothesis kernels) on
// the stream -- so the workspace keeps the size sosvo_[rgbd_]sequence_workspace has always answered.
template <typename Track>
uint64_t* pair_seeds(const Track& b) {
  return reinterpret_cast<uint64_t*>(b.lm_cost);
}

// The slot pairs of a sequence tracking call (entry point `fn`), checked against the store (host arrays: a bad slot would
// index outside the store on the device).  Up to kSeqArgPairs come back in `sp` for the setup kernel; larger
// batches are copied to b.ref_frame / b.cur_frame (pageable host memory: the copy returns when staged).
// seed_host (the ..._track_seeds entry points; nullptr otherwise): the pairs' seeds travel the same way, in `ps` or, copied,
// to pair_seeds(b).
template <typename Track>
int32_t upload_slot_pairs(sosvo_ctx* ctx, const char* fn, const int32_t* ref_slot, const int32_t* cur_slot,
                          const uint64_t* seed_host, int32_t n_pairs, int32_t slots, const Track& b, SlotPairs& sp,
                          PairSeeds& ps) {
  for (int i = 0; i < n_pairs; ++i)
    REQUIRE_FOR(ctx, fn, ref_slot[i] >= 0 && ref_slot[i] < slots && cur_slot[i] >= 0 && cur_slot[i] < slots, "slot out of range");
  for (int i = 0; i < kSeqArgPairs; ++i) {
    sp.ref[i] = i < n_pairs ? ref_slot[i] : 0;
    sp.cur[i] = i < n_pairs ? cur_slot[i] : 0;
    ps.seed[i] = seed_host && i < n_pairs ? seed_host[i] : 0;
  }
  if (n_pairs > kSeqArgPairs) {
    if (seed_host)
      SOSVO_HIP(ctx, hipMemcpyAsync(pair_seeds(b), seed_host, sizeof(uint64_t) * n_pairs, hipMemcpyHostToDevice, ctx->stream));
    SOSVO_HIP(ctx, hipMemcpyAsync(b.ref_frame, ref_slot, sizeof(int32_t) * n_pairs, hipMemcpyHostToDevice, ctx->stream));
    SOSVO_HIP(ctx, hipMemcpyAsync(b.cur_frame, cur_slot, sizeof(int32_t) * n_pairs, hipMemcpyHostToDevice, ctx->stream));
  }
  return SOSVO_OK;
}

// The (source, destination) lists of a ..._copy_slots call (entry point `fn`), checked on the host: slots of the store, no
// slot written twice, none both read and written (a launch copies all pairs at once).
int32_t check_copy_lists(sosvo_ctx* ctx, const char* fn, const int32_t* src, const int32_t* dst, int32_t n, int32_t slots,
                         CopyPairs& cp) {
  for (int i = 0; i < n; ++i)
    REQUIRE_FOR(ctx, fn, src[i] >= 0 && src[i] < slots && dst[i] >= 0 && dst[i] < slots, "slot out of range");
  const char* msg = "a slot is a destination twice, or both a source and a destination";
  if (n <= kSeqArgPairs) {  // (the serial round of up to 16 lanes: pairwise, nothing allocated)
    for (int i = 0; i < n; ++i) {
      for (int j = 0; j < n; ++j) REQUIRE_FOR(ctx, fn, dst[i] != src[j], msg);
      for (int j = 0; j < i; ++j) REQUIRE_FOR(ctx, fn, dst[i] != dst[j], msg);
    }
  } else {
    std::vector<uint8_t> use((size_t)slots, 0);  // 1: read, 2: written
    for (int i = 0; i < n; ++i) use[src[i]] = 1;
    for (int i = 0; i < n; ++i) {
      REQUIRE_FOR(ctx, fn, use[dst[i]] == 0, msg);
      use[dst[i]] = 2;
    }
  }
  for (int i = 0; i < kSeqArgPairs; ++i) {
    cp.src[i] = i < n ? src[i] : 0;
    cp.dst[i] = i < n ? dst[i] : 0;
  }
  return SOSVO_OK;
}

// The slot table of a ..._front_end_slots call (entry point `fn`): slots of the store, none twice (a bad table would write
// outside the store, or two frames' records over each other).  Once per window of frames, not per serial call; small
// tables are compared pairwise, larger ones marked in a host array.
int32_t check_slot_table(sosvo_ctx* ctx, const char* fn, const int32_t* slot_of_frame, int32_t n, int32_t slots) {
  for (int i = 0; i < n; ++i) REQUIRE_FOR(ctx, fn, slot_of_frame[i] >= 0 && slot_of_frame[i] < slots, "slot out of range");
  const char* msg = "a slot appears twice in slot_of_frame";
  if (n <= 64) {
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < i; ++j) REQUIRE_FOR(ctx, fn, slot_of_frame[i] != slot_of_frame[j], msg);
    return SOSVO_OK;
  }
  std::vector<uint8_t> used((size_t)slots, 0);
  for (int i = 0; i < n; ++i) {
    REQUIRE_FOR(ctx, fn, !used[slot_of_frame[i]], msg);
    used[slot_of_frame[i]] = 1;
  }
  return SOSVO_OK;
}

}  // namespace

extern "C" {

size_t sosvo_frame_pair_batch_workspace(const sosvo_batch_cfg* cfg) {
  if (!cfg || cfg->n_pairs <= 0 || cfg->rows <= 0 || cfg->cols <= 0 || cfg->nmask <= 0 || cfg->kp_cap <= 0 ||
      cfg->frame_cap <= 0 || !detector_ok(cfg->detector, cfg->kp_cap) || omni_flags_msg(*cfg) ||
      (lk_f2f(*cfg) && cfg->n_pairs > 8192))  // (the store's images: 2 * slots <= 65535)
    return 0;
  // (laxer than the call itself, which refuses nmask > 32, kp_cap > 4096 and frame_cap > 16384: such a shape gets a size
  // here and "out of range" there)
  const size_t F = 2 * (size_t)cfg->n_pairs;
  return carve(*cfg, F, F, nullptr, true).bytes;
}

#define STAGE(call)              \
  do {                           \
    rc = (call);                 \
    if (rc != SOSVO_OK) return rc; \
  } while (0)

// The slot tables of a matching step of n problems with the mutual-consistency filter.  q / t: the tracking call's device
// slot pairs (nullptr: static stereo, see mutual_tabs_kernel).
static int32_t mutual_tabs(sosvo_ctx* ctx, const int32_t* q, const int32_t* t, int n, const MutualTabs& m) {
  SOSVO_LAUNCH(ctx, mutual_tabs_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, n, q, t, m.q_slot, m.t_slot);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

// The 1-NN search of a matching step: under the gate g when it is on (positions q_pos / t_pos, indexed like the descriptors;
// problems at and beyond n_forward have the roles swapped), plain otherwise; with the ratio rule r on the forward problems
// when it is on.
static int32_t match_1nn(sosvo_ctx* ctx, const Gate& g, const Ratio& r, const uint8_t* q_desc, const uint8_t* t_desc, const float* q_pos,
                         const float* t_pos, const int32_t* nq, const int32_t* nt, const int32_t* q_slot, const int32_t* t_slot,
                         int nprob, int n_forward, int stride, uint32_t* keys) {
  if (r.r64)
    return sosvo_match_hamming_ratio(ctx, q_desc, t_desc, g.on ? q_pos : nullptr, g.on ? t_pos : nullptr, nq, nt, q_slot, t_slot,
                                     nprob, n_forward, stride, stride, g.min_dv, g.max_du, g.on ? g.max_distance : 256, r.r64,
                                     keys, r.rivals);
  if (!g.on) return sosvo_match_hamming(ctx, q_desc, t_desc, nq, nt, q_slot, t_slot, nprob, stride, stride, 1, keys);
  if (g.period > 0.0)
    return sosvo_match_hamming_gated_cyclic(ctx, q_desc, t_desc, q_pos, t_pos, nq, nt, q_slot, t_slot, nprob, n_forward, stride,
                                            stride, g.max_du, g.period, g.max_distance, keys);
  return sosvo_match_hamming_gated(ctx, q_desc, t_desc, q_pos, t_pos, nq, nt, q_slot, t_slot, nprob, n_forward, stride, stride,
                                   g.min_dv, g.max_du, g.max_distance, keys);
}

// One such step over the descriptor store `desc` (blocks of `stride` rows, counts `cnt`, positions `pos`): ONE launch of n
// forward + n role-swapped problems through the tables, then the filter on the forward keys.  The forward keys of `keys`
// [2 n, stride] are sorted and assembled like those of a plain sosvo_match_hamming call.
static int32_t match_mutual(sosvo_ctx* ctx, const Gate& g, const Ratio& r, const uint8_t* desc, const float* pos, const int32_t* cnt, int n,
                            int stride, const MutualTabs& m, uint32_t* keys) {
  int32_t rc;
  STAGE(match_1nn(ctx, g, r, desc, desc, pos, pos, cnt, cnt, m.q_slot, m.t_slot, 2 * n, n, stride, keys));
  return sosvo_cross_check_matches(ctx, keys, keys + (size_t)n * stride, cnt, cnt, m.q_slot, m.t_slot, n, stride, stride, keys,
                                   nullptr);
}

// The image front end + static stereo of F frames (OmniStereoModel.set_current_omni_image + StereoPanoramicFrame.__init__,
// camera_models.py:3107-3120, pose_est_tools.py:271-402): K1, K2 + K3, K4, K6 over all 2 F panoramas, per-bucket top/bottom
// matching, gates, bearings, midpoint triangulation, range filter -> F frame records written at out_* (frame-major).
static int32_t run_front_end(sosvo_ctx* ctx, const sosvo_rig* rig, const sosvo_batch_cfg* cfg, int F, const uint8_t* omni,
                             const uint32_t* unwrap_table, const uint32_t* mask_bits, const int8_t* pattern,
                             const FrontEndTmp& t, const FrameStore& o, hipEvent_t median_wait, hipEvent_t median_done,
                             const int32_t* slot_of_frame = nullptr, const Workspace* images = nullptr, int first_slot = 0) {
  const int NI = 2 * F, NM = cfg->nmask, cap = cfg->kp_cap, Fc = cfg->frame_cap;
  const int h = F * NM;  // problems of one view: (frame, mask); the top view's come first (view-major images)
  const int cols = run_cols(*cfg);  // the columns of the image stages: the period, or the padded panorama (SOSVO_FLAG_SEAM_FREE)
  int32_t rc;
  SOSVO_REQUIRE(ctx, seam_free_stereo_lk_ok(*cfg, ctx->stereo_lk), kBadSeamStereoLk);
  if (median_wait) SOSVO_HIP(ctx, hipStreamWaitEvent(ctx->stream, median_wait, 0));
  const int det = cfg->detector;
  const bool fused_median = cfg->median_ksize == 3 || cfg->median_ksize == 5 || cfg->median_ksize == 11;
  // skipping unreachable rows is exact for GFT only (the range is GFT's reach); ORB, FAST and AGAST see every row, as
  // ImageFrontEnd computes them
  const bool rows_known = gray_rows_known(*cfg);
  if (rows_known) {
    // rows beyond the reach of GFT on the masks and of ORB.compute on its keypoints are not computed (the range is a
    // model constant; a 2-workgroup kernel per call keeps this entry point free of caller-side state)
    STAGE(sosvo_gray_rows_needed(ctx, mask_bits, 2, cfg->rows, cols, NM, cfg->edge, pattern, cfg->cos_a, cfg->sin_a,
                                 t.gray_rows));
    STAGE(sosvo_unwrap_median_gray_rows(ctx, omni, unwrap_table, F, cfg->H, cfg->W, cfg->rows, cols, cfg->median_ksize,
                                        t.gray_rows, t.gray));
  } else if (cfg->median_ksize <= 1 || fused_median) {  // every row (ksize <= 1: unwrap straight to gray)
    STAGE(sosvo_unwrap_median_gray_rows(ctx, omni, unwrap_table, F, cfg->H, cfg->W, cfg->rows, cols, cfg->median_ksize,
                                        nullptr, t.gray));
  } else {
    STAGE(sosvo_unwrap_table(ctx, omni, unwrap_table, F, cfg->H, cfg->W, cfg->rows, cols, t.pano));
    STAGE(sosvo_median_gray(ctx, t.pano, NI, cfg->rows, cols, cfg->median_ksize, t.gray));
  }
  if (median_done) SOSVO_HIP(ctx, hipEventRecord(median_done, ctx->stream));
  // SOSVO_FLAG_LK_F2F: the frames' gray rows and the pyramid levels in use go where their records go (`images`: the workspace
  // whose store `o` belongs to, o shifted by first_slot)
  if (images && images->img.level[0])
    STAGE(sosvo_lk_images_fill(ctx, images->img, ctx->lk.levels, images->img_rows, images->img_in_place ? nullptr : t.gray, F,
                               first_slot, slot_of_frame, cyclic_f2f(*cfg), seam_free(*cfg) ? SOSVO_SEAM_HALO : 0));
  // the stages ImageFrontEnd.run_features calls for the detector (frontend.py), with the same arguments
  if (det == SOSVO_DETECTOR_ORB) {
    // the mask pyramid is a model constant, rebuilt here on every call (as gray_rows above) to keep the entry point free of
    // caller-side state; kp_xy (level-0 x, y of the compacted keypoints) feeds the matching, each keypoint keeps its angle
    STAGE(sosvo_orb_mask_pyramid(ctx, mask_bits, 2, cfg->rows, cols, NM, t.orb.mask_pyr));
    STAGE(sosvo_detect_describe_orb(ctx, t.gray, t.orb.mask_pyr, NI, F, cfg->rows, cols, NM, cfg->max_corners, cap,
                                    t.orb.kp4, t.orb.resp, t.n, pattern, t.desc, t.kp));
  } else if (det == SOSVO_DETECTOR_FAST || det == SOSVO_DETECTOR_AGAST) {
    STAGE((det == SOSVO_DETECTOR_FAST ? sosvo_detect_fast : sosvo_detect_agast)(ctx, t.gray, mask_bits, NI, F, cfg->rows,
                                                                                cols, NM, 10, cap, t.kp, t.n, t.status));
    STAGE(sosvo_describe_orb_rows(ctx, t.gray, NI, cfg->rows, cols, NM, cap, t.kp, t.n, cfg->cos_a, cfg->sin_a, pattern,
                                  cfg->edge, nullptr, t.desc));
  } else {
    STAGE(sosvo_detect_gft(ctx, t.gray, mask_bits, NI, F, cfg->rows, cols, NM, cfg->quality, cfg->min_distance,
                           cfg->max_corners, cap, t.kp, t.n, t.status));
    STAGE(sosvo_describe_orb_rows(ctx, t.gray, NI, cfg->rows, cols, NM, cap, t.kp, t.n, cfg->cos_a, cfg->sin_a, pattern,
                                  cfg->edge, rows_known ? t.gray_rows : nullptr, t.desc));
  }
  // sub-pixel refinement (SOSVO_FLAG_SUBPIX) where ImageFrontEnd.run_features has it: the descriptors above are those of the
  // detector's positions, everything below sees the refined ones (ORB: kp_xy; kp4 keeps the detector's)
  if (cfg->ransac_flags & SOSVO_FLAG_SUBPIX)
    STAGE(sosvo_refine_subpix(ctx, t.gray, NI, cfg->rows, cols, NM, cap, t.kp, t.n, SOSVO_SUBPIX_HALF_OF(cfg->ransac_flags), 10,
                              0.01, rows_known ? t.gray_rows : nullptr));
  // static stereo per frame: query = bottom view, train = top view, bucket by bucket
  const float *kp_top = t.kp, *kp_bot = t.kp + (size_t)h * cap * 2;
  const uint8_t *desc_top = t.desc, *desc_bot = t.desc + (size_t)h * cap * 32;
  const int32_t *n_top = t.n, *n_bot = t.n + h;
  const Gate gate = gate_stereo(*cfg, *rig);
  if (cross_stereo(*cfg)) {  // (top and bottom are the two halves of t.desc / t.kp / t.n: blocks p and h + p)
    STAGE(mutual_tabs(ctx, nullptr, nullptr, h, t.mutual));
    STAGE(match_mutual(ctx, gate, t.ratio, t.desc, t.kp, t.n, h, cap, t.mutual, t.s_keys));
  } else
    STAGE(match_1nn(ctx, gate, t.ratio, desc_bot, desc_top, kp_bot, kp_top, n_bot, n_top, nullptr, nullptr, h, h, cap, t.s_keys));
  STAGE(sosvo_sort_matches(ctx, t.s_keys, n_bot, nullptr, h, cap, t.s_order));
  // sub-pixel static stereo (SOSVO_FLAG_LK_STEREO): the bottom keypoint of every matched pair moves to where the top one's
  // window is found in the bottom panorama; the gates, bearings, triangulation and m_bot below see the refined positions
  if (lk_stereo(*cfg))
    STAGE(sosvo_refine_stereo_lk(ctx, t.gray, NI, cfg->rows, cols, rows_known ? t.gray_rows : nullptr, NM, cap, kp_top, n_top,
                                 t.kp + (size_t)h * cap * 2, n_bot, t.s_keys, rig->stereo_min_disp, rig->stereo_max_hdiff, nullptr,
                                 t.lk_status));
  // SOSVO_FLAG_SEAM_FREE: everything above ran in the padded panoramas' coordinates; the assemble, the store and the tracking
  // step see the period's columns (both views' keypoints: they are the two halves of t.kp)
  if (seam_free(*cfg)) STAGE(sosvo_keypoints_unpad(ctx, t.kp, t.n, 2 * h, cap, cfg->cols));
  if (slot_of_frame)  // (HOST table: frame i's record goes to record slot_of_frame[i] of o)
    STAGE(sosvo_stereo_assemble_slots(ctx, rig, kp_top, kp_bot, desc_top, desc_bot, n_top, n_bot, t.s_keys, t.s_order, F,
                                      slot_of_frame, NM, cap, Fc, o.m_top, o.m_bot, o.d_top, o.d_bot, o.X, o.b_top, o.b_bot, o.M,
                                      t.n_cand));
  else
    STAGE(sosvo_stereo_assemble(ctx, rig, kp_top, kp_bot, desc_top, desc_bot, n_top, n_bot, t.s_keys, t.s_order, F, NM, cap,
                                Fc, o.m_top, o.m_bot, o.d_top, o.d_bot, o.X, o.b_top, o.b_bot, o.M, t.n_cand));
  return SOSVO_OK;
}

// The frame-to-frame correspondences of B slot pairs by MATCHING: per view query = current frame, train = reference frame, sort,
// |du| gate, stacking (b.f, b.p, b.cam, b.cq, b.ct, b.cn, b.cn_top).
static int32_t correspondences_matched(sosvo_ctx* ctx, const sosvo_rig* rig, const sosvo_batch_cfg* cfg, int B, const FrameStore& s,
                                       const TrackTmp& b) {
  const int Fc = cfg->frame_cap, Cc = 2 * Fc;
  int32_t rc;
  const bool mutual = cross_f2f(*cfg), cyclic = cyclic_f2f(*cfg);
  const Gate gate = gate_f2f(*cfg, *rig);
  Gate gate_bot = gate;
  if (cyclic && gate.on) {  // the view's period; the entry point refuses a period that is no positive integer
    SOSVO_REQUIRE(ctx, rig->pano_top[0] >= 1.0 && rig->pano_bot[0] >= 1.0, "SOSVO_FLAG_CYCLIC_F2F: the period (pano_top[0], pano_bot[0]) must be positive");
    gate_bot.period = rig->pano_bot[0];
  }
  Gate gate_top = gate_bot;
  gate_top.period = cyclic && gate.on ? rig->pano_top[0] : 0.0;
  if (mutual) {  // (one pair of tables serves both views)
    STAGE(mutual_tabs(ctx, b.cur_frame, b.ref_frame, B, b.mutual));
    STAGE(match_mutual(ctx, gate_top, b.ratio, s.d_top, s.m_top, s.M, B, Fc, b.mutual, b.k_top));
  } else
    STAGE(match_1nn(ctx, gate_top, b.ratio, s.d_top, s.d_top, s.m_top, s.m_top, s.M, s.M, b.cur_frame, b.ref_frame, B, B, Fc, b.k_top));
  STAGE(sosvo_sort_matches(ctx, b.k_top, s.M, b.cur_frame, B, Fc, b.o_top));
  if (mutual)
    STAGE(match_mutual(ctx, gate_bot, b.ratio, s.d_bot, s.m_bot, s.M, B, Fc, b.mutual, b.k_bot));
  else
    STAGE(match_1nn(ctx, gate_bot, b.ratio, s.d_bot, s.d_bot, s.m_bot, s.m_bot, s.M, s.M, b.cur_frame, b.ref_frame, B, B, Fc, b.k_bot));
  STAGE(sosvo_sort_matches(ctx, b.k_bot, s.M, b.cur_frame, B, Fc, b.o_bot));
  return (cyclic ? sosvo_f2f_assemble_cyclic : sosvo_f2f_assemble)(ctx, rig, s.m_top, s.m_bot, s.X, s.b_top, s.b_bot, s.M, Fc, b.ref_frame, b.cur_frame, b.k_top, b.o_top,
                            b.k_bot, b.o_bot, B, Cc, b.f, b.p, b.cam, b.cq, b.ct, b.cn, b.cn_top);
}

// ... by TRACKING (SOSVO_FLAG_LK_F2F): the reference frames' points, read where the store keeps them, followed into the current
// frames' images with the context's settings -- ONE tracker launch of 2 B problems, top views first -- then the tracked
// assemble into the same outputs.
static int32_t correspondences_tracked(sosvo_ctx* ctx, const sosvo_rig* rig, const sosvo_batch_cfg* cfg, int B, const FrameStore& s,
                                       const TrackTmp& b, const sosvo_lk_images& im, const int32_t* img_rows) {
  const int Fc = cfg->frame_cap, Cc = 2 * Fc;
  int32_t rc;
  const LkTmp& k = b.lk;
  SOSVO_REQUIRE(ctx, im.level[0] && k.next, "SOSVO_FLAG_LK_F2F without the store's images");
  SOSVO_LAUNCH(ctx, lk_setup_kernel, dim3(cdiv(2 * B, 256)), dim3(256), 0, ctx->stream, B, im.slots, Fc, b.ref_frame, b.cur_frame, s.M,
               (int64_t)((s.m_bot - s.m_top) / 2), k.from, k.to, k.n, k.pt);
  SOSVO_LAUNCH_CHECK(ctx);
  const bool cyclic = cyclic_f2f(*cfg);
  STAGE(sosvo_lk_images_track(ctx, im, ctx->lk, img_rows, k.from, k.to, 2 * B, Fc, s.m_top, k.pt, k.n, k.next, k.status, k.err, k.back,
                              cyclic));
  return (cyclic ? sosvo_f2f_assemble_tracked_cyclic : sosvo_f2f_assemble_tracked)(ctx, rig, s.m_top, s.m_bot, s.X, s.M, Fc, b.ref_frame, k.next, k.next + (size_t)B * Fc * 2, k.status,
                                    k.status + (size_t)B * Fc, B, Cc, b.f, b.p, b.cam, b.cq, b.ct, b.cn, b.cn_top);
}

// TrackerStereoSE3.track_frame (pose_est_tools.py:736-847) for B (reference slot, current slot) pairs of a frame store:
// frame-to-frame matching per view (query = current frame, train = reference frame), |du| gate, stacking -- or the tracker in
// the matcher's place (`images`: the workspace the store belongs to, for its images) --, non-central
// RANSAC (problem i samples with seed + i), LM on the inliers, [B,16] records.
// (seeds: device array of per-pair seeds, pair i samples with seeds[i]; nullptr: with seed + i)
static int32_t run_tracking(sosvo_ctx* ctx, const sosvo_rig* rig, const sosvo_batch_cfg* cfg, int B, uint64_t seed,
                            const FrameStore& s, const TrackTmp& b, double* results, const uint64_t* seeds = nullptr,
                            const Workspace* images = nullptr) {
  const int Fc = cfg->frame_cap, Cc = 2 * Fc;
  int32_t rc;
  SOSVO_REQUIRE(ctx, !lk_f2f(*cfg) || images, "SOSVO_FLAG_LK_F2F without the store's images");
  if (lk_f2f(*cfg))
    STAGE(correspondences_tracked(ctx, rig, cfg, B, s, b, images->img, images->img_rows));
  else
    STAGE(correspondences_matched(ctx, rig, cfg, B, s, b));
  // 3D-2D absolute pose: RANSAC, then LM on the inliers
  const int32_t rflags = SOSVO_FLAG_CAM_ROT_IDENTITY | (cfg->ransac_flags & SOSVO_FLAG_GP3P);
  if (seeds)
    STAGE(sosvo_ransac_abs_pose_seeds(ctx, b.f, b.p, b.cam, b.cam_off, b.cam_rot, 2, rflags, b.cn, B, Cc, cfg->ransac_threshold,
                                      cfg->ransac_max_iter, cfg->ransac_adaptive, seeds, b.T_ransac, b.mask, b.idx, b.n_inl,
                                      b.info, nullptr));
  else
    STAGE(sosvo_ransac_abs_pose(ctx, b.f, b.p, b.cam, b.cam_off, b.cam_rot, 2, rflags, b.cn, B, Cc, cfg->ransac_threshold,
                                cfg->ransac_max_iter, cfg->ransac_adaptive, seed, b.T_ransac, b.mask, b.idx, b.n_inl, b.info,
                                nullptr));
  SOSVO_HIP(ctx, hipMemcpyAsync(b.T, b.T_ransac, sizeof(double) * 12 * B, hipMemcpyDeviceToDevice, ctx->stream));
  STAGE(sosvo_refine_abs_pose(ctx, b.f, b.p, b.cam, b.cam_off, b.cam_rot, 2, b.cn, B, Cc, b.idx, b.n_inl, cfg->lm_max_iter,
                              b.T, b.lm_cost, b.lm_iters));
  SOSVO_LAUNCH(ctx, batch_results_kernel, dim3(cdiv(B, 256)), dim3(256), 0, ctx->stream, B, b.T, b.n_inl, b.cn, b.info,
               results);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

// (median_wait / median_done: the token that serialises the VALU-bound median launches of the parts of a multi-stream
// batch, see sosvo_frame_pair_batch_streams; nullptr for a plain call)
static int32_t run_frame_pairs(sosvo_ctx* ctx, const sosvo_rig* rig, const sosvo_batch_cfg* cfg, const uint8_t* omni,
                               const uint32_t* unwrap_table, const uint32_t* mask_bits, const int8_t* pattern,
                               void* workspace, size_t workspace_bytes, double* results, hipEvent_t median_wait,
                               hipEvent_t median_done) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, rig && cfg && omni && unwrap_table && mask_bits && pattern && workspace && results, "null pointer");
  SOSVO_REQUIRE(ctx, cfg->n_pairs > 0 && cfg->n_pairs <= 8192, "n_pairs out of range (1..8192)");
  SOSVO_REQUIRE(ctx, cfg->nmask >= 1 && cfg->nmask <= 32 && cfg->kp_cap > 0 && cfg->kp_cap <= 4096, "nmask / kp_cap out of range");
  SOSVO_REQUIRE(ctx, cfg->frame_cap > 0 && cfg->frame_cap <= 16384, "frame_cap out of range (max 16384)");
  SOSVO_REQUIRE(ctx, detector_ok(cfg->detector, cfg->kp_cap), "unknown detector, or ORB with kp_cap > 2048");
  if (omni_flags_msg(*cfg)) return sosvo_fail(ctx, SOSVO_ERR_ARG, __func__, omni_flags_msg(*cfg));
  SOSVO_REQUIRE(ctx, !lk_f2f(*cfg) || sosvo_lk_options_ok(ctx->lk), "LK settings out of range (sosvo_set_lk_options)");
  SOSVO_REQUIRE(ctx, ((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
  const int B = cfg->n_pairs, F = 2 * B;
  const Workspace ws = carve(*cfg, F, F, workspace, true);
  SOSVO_REQUIRE(ctx, workspace_bytes >= ws.bytes, "workspace too small (see sosvo_frame_pair_batch_workspace)");
  int32_t rc;
  SOSVO_LAUNCH(ctx, batch_setup_kernel, dim3(cdiv(B > 18 ? B : 18, 256)), dim3(256), 0, ctx->stream, B, foci_of(rig),
               ws.tt.ref_frame, ws.tt.cur_frame, ws.tt.cam_off, ws.tt.cam_rot);
  SOSVO_LAUNCH_CHECK(ctx);
  STAGE(run_front_end(ctx, rig, cfg, F, omni, unwrap_table, mask_bits, pattern, ws.fe, ws.store, median_wait, median_done, nullptr,
                      &ws));
  return run_tracking(ctx, rig, cfg, B, cfg->seed, ws.store, ws.tt, results, nullptr, &ws);
}

int32_t sosvo_frame_pair_batch(sosvo_ctx* ctx, const sosvo_rig* rig, const sosvo_batch_cfg* cfg, const uint8_t* omni,
                               const uint32_t* unwrap_table, const uint32_t* mask_bits, const int8_t* pattern,
                               void* workspace, size_t workspace_bytes, double* results) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, rig && cfg && omni && unwrap_table && mask_bits && pattern && workspace && results, "null pointer");
  SOSVO_REQUIRE(ctx, sosvo_table_frame_ok(cfg->H, cfg->W), SOSVO_TABLE_FRAME_MSG);
  return run_frame_pairs(ctx, rig, cfg, omni, unwrap_table, mask_bits, pattern, workspace, workspace_bytes, results, nullptr,
                         nullptr);
}

// ---- the same batch split over internal HIP streams ------------------------------------------------------
static void part_range(int n, int part, int parts, int* lo, int* hi) {  // contiguous blocks, sizes differ by at most one
  const int base = n / parts, extra = n % parts;
  *lo = part * base + (part < extra ? part : extra);
  *hi = *lo + base + (part < extra ? 1 : 0);
}

size_t sosvo_frame_pair_batch_streams_workspace(const sosvo_batch_cfg* cfg, int32_t n_streams) {
  if (!cfg || n_streams < 1 || n_streams > kSosvoMaxSubStreams || cfg->n_pairs < n_streams) return 0;
  size_t total = 0;
  for (int s = 0; s < n_streams; ++s) {
    int lo, hi;
    part_range(cfg->n_pairs, s, n_streams, &lo, &hi);
    sosvo_batch_cfg c = *cfg;
    c.n_pairs = hi - lo;
    const size_t bytes = sosvo_frame_pair_batch_workspace(&c);
    if (bytes == 0) return 0;
    total += sosvo_round256(bytes);
  }
  return total;
}

static int32_t sosvo_frame_pair_batch_streams_impl(sosvo_ctx* ctx, const sosvo_rig* rig, const sosvo_batch_cfg* cfg, int32_t n_streams,
                             const uint8_t* omni, const uint32_t* unwrap_table, const uint32_t* mask_bits,
                             const int8_t* pattern, void* workspace, size_t workspace_bytes, double* results, bool join) {
  SOSVO_REQUIRE(ctx, n_streams >= 1 && n_streams <= kSosvoMaxSubStreams, "n_streams out of range (1..4)");
  SOSVO_REQUIRE(ctx, cfg->n_pairs >= n_streams && cfg->n_pairs <= 8192, "n_pairs out of range (n_streams..8192)");
  SOSVO_REQUIRE(ctx, detector_ok(cfg->detector, cfg->kp_cap), "unknown detector, or ORB with kp_cap > 2048");
  if (omni_flags_msg(*cfg)) return sosvo_fail(ctx, SOSVO_ERR_ARG, __func__, omni_flags_msg(*cfg));
  SOSVO_REQUIRE(ctx, ((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
  const size_t need = sosvo_frame_pair_batch_streams_workspace(cfg, n_streams);
  SOSVO_REQUIRE(ctx, need > 0 && workspace_bytes >= need, "workspace too small (see sosvo_frame_pair_batch_streams_workspace)");
  // internal sub-contexts: one stream and one scratch workspace each, created on first use, kept for the context's life
  while (ctx->n_sub < n_streams) {
    const int i = ctx->n_sub;
    if (i == 0) SOSVO_HIP(ctx, hipEventCreateWithFlags(&ctx->sub_begin, hipEventDisableTiming));
    hipStream_t st;
    SOSVO_HIP(ctx, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    const int32_t rc = sosvo_create(&ctx->sub[i], ctx->device, st);
    if (rc != SOSVO_OK) {
      (void)hipStreamDestroy(st);
      return sosvo_fail(ctx, rc, __func__, "cannot create an internal stream context");
    }
    ctx->sub[i]->hint_shared_device = 1;  // the parts run side by side
    ctx->sub[i]->hint_score_fp64_only = ctx->hint_score_fp64_only;
    ctx->sub[i]->hint_rolling_narrow = ctx->hint_rolling_narrow;
    SOSVO_HIP(ctx, hipEventCreateWithFlags(&ctx->sub_done[i], hipEventDisableTiming));
    SOSVO_HIP(ctx, hipEventCreateWithFlags(&ctx->sub_median[i], hipEventDisableTiming));
    ctx->n_sub = i + 1;
  }
  // the slice layout of this call: part s uses bytes[s] from workspace + bytes[0] + ... + bytes[s - 1].  A part's size
  // depends on the whole configuration (detector, kp_cap, nmask, frame_cap, rows / cols, H / W, ...), not only on its pairs
  size_t bytes[kSosvoMaxSubStreams];
  for (int s = 0; s < n_streams; ++s) {
    int lo, hi;
    part_range(cfg->n_pairs, s, n_streams, &lo, &hi);
    sosvo_batch_cfg c = *cfg;
    c.n_pairs = hi - lo;
    bytes[s] = sosvo_round256(sosvo_frame_pair_batch_workspace(&c));
  }
  if (ctx->sub_pending) {
    // un-joined parts of an earlier ..._enqueue call may still run.  A stream capture cannot depend on them (their events
    // were recorded outside it), and a different slice layout would lay this call's slices over slices an earlier part
    // still uses on ANOTHER stream (a slice is ordered by its own part stream only): join first in both cases.
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    SOSVO_HIP(ctx, hipStreamIsCapturing(ctx->stream, &cap));
    SOSVO_REQUIRE(ctx, cap == hipStreamCaptureStatusNone,
                  "un-joined sosvo_frame_pair_batch_streams_enqueue work is pending: call ..._join before capturing");
    bool same = ctx->sub_last == n_streams && ctx->sub_last_ws == workspace;
    for (int s = 0; same && s < n_streams; ++s) same = ctx->sub_last_bytes[s] == bytes[s];
    if (!same) {
      for (int s = 0; s < ctx->sub_last; ++s) SOSVO_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->sub_done[s], 0));
      ctx->sub_pending = 0;
    }
  }
  // every part starts after the work already queued on the caller's stream ...
  SOSVO_HIP(ctx, hipEventRecord(ctx->sub_begin, ctx->stream));
  char* ws = reinterpret_cast<char*>(workspace);
  // ... and the medians take turns: part s waits for the median of part s - 1; the first part waits for the LAST part of
  // the previous call only while that call is un-joined (back-to-back ..._enqueue calls).  After a join the chain starts
  // afresh: everything earlier is already ordered before sub_begin, and an event recorded before a stream capture began
  // must not be waited on inside it.
  hipEvent_t token = (ctx->sub_pending && ctx->sub_last > 0) ? ctx->sub_median[ctx->sub_last - 1] : nullptr;
  for (int s = 0; s < n_streams; ++s) {
    int lo, hi;
    part_range(cfg->n_pairs, s, n_streams, &lo, &hi);
    sosvo_batch_cfg c = *cfg;
    c.n_pairs = hi - lo;
    c.seed = cfg->seed + (uint64_t)lo;  // pair i samples with seed + i, whatever the split
    sosvo_ctx* sc = ctx->sub[s];
    sc->lk = ctx->lk;  // (settings, not hints: they change results, so every part tracks with the caller's)
    sc->stereo_lk = ctx->stereo_lk;
    SOSVO_HIP(ctx, hipStreamWaitEvent(sc->stream, ctx->sub_begin, 0));
    const int32_t rc = run_frame_pairs(sc, rig, &c, omni + (size_t)2 * lo * cfg->H * cfg->W * 3, unwrap_table, mask_bits, pattern,
                                       ws, bytes[s], results + (size_t)16 * lo, token, ctx->sub_median[s]);
    if (rc != SOSVO_OK) {
      // the parts launched so far (and whatever this one enqueued before failing) still run: the caller's stream must
      // not overtake them
      (void)hipEventRecord(ctx->sub_done[s], sc->stream);
      for (int k = 0; k <= s; ++k) (void)hipStreamWaitEvent(ctx->stream, ctx->sub_done[k], 0);
      if (ctx->sub_pending)  // parts of the previous un-joined call beyond s: the caller's stream waits for them as well
        for (int k = s + 1; k < ctx->sub_last; ++k) (void)hipStreamWaitEvent(ctx->stream, ctx->sub_done[k], 0);
      ctx->sub_pending = 0;
      return sosvo_fail(ctx, rc, __func__, sc->err);
    }
    token = ctx->sub_median[s];
    SOSVO_HIP(ctx, hipEventRecord(ctx->sub_done[s], sc->stream));
    ws += bytes[s];
  }
  ctx->sub_last = n_streams;
  ctx->sub_last_ws = workspace;
  for (int s = 0; s < n_streams; ++s) ctx->sub_last_bytes[s] = bytes[s];
  ctx->sub_pending = join ? 0 : 1;
  // ... and the caller's stream continues after all of them
  if (join)
    for (int s = 0; s < n_streams; ++s) SOSVO_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->sub_done[s], 0));
  return SOSVO_OK;
}

int32_t sosvo_frame_pair_batch_streams(sosvo_ctx* ctx, const sosvo_rig* rig, const sosvo_batch_cfg* cfg, int32_t n_streams,
                                       const uint8_t* omni, const uint32_t* unwrap_table, const uint32_t* mask_bits,
                                       const int8_t* pattern, void* workspace, size_t workspace_bytes, double* results) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, rig && cfg && omni && unwrap_table && mask_bits && pattern && workspace && results, "null pointer");
  SOSVO_REQUIRE(ctx, sosvo_table_frame_ok(cfg->H, cfg->W), SOSVO_TABLE_FRAME_MSG);
  return sosvo_frame_pair_batch_streams_impl(ctx, rig, cfg, n_streams, omni, unwrap_table, mask_bits, pattern, workspace, workspace_bytes, results, true);
}

int32_t sosvo_frame_pair_batch_streams_enqueue(sosvo_ctx* ctx, const sosvo_rig* rig, const sosvo_batch_cfg* cfg,
                                               int32_t n_streams, const uint8_t* omni, const uint32_t* unwrap_table,
                                               const uint32_t* mask_bits, const int8_t* pattern, void* workspace,
                                               size_t workspace_bytes, double* results) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, rig && cfg && omni && unwrap_table && mask_bits && pattern && workspace && results, "null pointer");
  SOSVO_REQUIRE(ctx, sosvo_table_frame_ok(cfg->H, cfg->W), SOSVO_TABLE_FRAME_MSG);
  return sosvo_frame_pair_batch_streams_impl(ctx, rig, cfg, n_streams, omni, unwrap_table, mask_bits, pattern, workspace, workspace_bytes, results, false);
}

int32_t sosvo_frame_pair_batch_streams_join(sosvo_ctx* ctx) {
  SOSVO_ENTER(ctx);
  for (int s = 0; s < ctx->sub_last; ++s) SOSVO_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->sub_done[s], 0));
  ctx->sub_pending = 0;
  return SOSVO_OK;
}

size_t sosvo_rgbd_pair_batch_workspace(const sosvo_rgbd_batch_cfg* cfg) {
  if (!cfg || cfg->n_pairs <= 0 || cfg->rows <= 0 || cfg->cols <= 0 || cfg->kp_cap <= 0 || cfg->frame_cap <= 0 ||
      !detector_ok(rgbd_detector(*cfg), cfg->kp_cap) || !rgbd_flags_ok(*cfg))
    return 0;
  const size_t F = 2 * (size_t)cfg->n_pairs;
  return carve_rgbd(*cfg, F, F, nullptr).bytes;
}

// RGBDFrame.establish_keypoints for F frames (pose_est_tools.py:600-623): [median,] gray, whole-image detection (one mask;
// GFT, ORB, FAST or AGAST), ORB descriptors, depth back-projection + range filter + bearings -> F frame records at the store
// pointers.
static int32_t run_rgbd_front_end(sosvo_ctx* ctx, const sosvo_rgbd_cam* cam, const sosvo_rgbd_batch_cfg* cfg, int F,
                                  const uint8_t* bgr, const float* depth, const uint32_t* mask_bits, const int8_t* pattern,
                                  const RgbdFrontTmp& t, const RgbdStore& o, const int32_t* slot_of_frame = nullptr) {
  const int cap = cfg->kp_cap, Fc = cfg->frame_cap;
  int32_t rc;
  const int det = rgbd_detector(*cfg);
  STAGE(sosvo_median_gray(ctx, bgr, F, cfg->rows, cfg->cols, cfg->median_ksize, t.gray));
  if (det == SOSVO_DETECTOR_ORB) {  // (the mask pyramid: a model constant rebuilt per call, as in run_front_end)
    STAGE(sosvo_orb_mask_pyramid(ctx, mask_bits, 1, cfg->rows, cfg->cols, 1, t.orb.mask_pyr));
    STAGE(sosvo_detect_describe_orb(ctx, t.gray, t.orb.mask_pyr, F, F, cfg->rows, cfg->cols, 1, cfg->max_corners, cap, t.orb.kp4,
                                    t.orb.resp, t.n, pattern, t.desc, t.kp));
  } else {
    if (det == SOSVO_DETECTOR_FAST || det == SOSVO_DETECTOR_AGAST)
      STAGE((det == SOSVO_DETECTOR_FAST ? sosvo_detect_fast : sosvo_detect_agast)(ctx, t.gray, mask_bits, F, F, cfg->rows, cfg->cols,
                                                                                  1, 10, cap, t.kp, t.n, t.status));
    else
      STAGE(sosvo_detect_gft(ctx, t.gray, mask_bits, F, F, cfg->rows, cfg->cols, 1, cfg->quality, cfg->min_distance,
                             cfg->max_corners, cap, t.kp, t.n, t.status));
    STAGE(sosvo_describe_orb(ctx, t.gray, F, cfg->rows, cfg->cols, 1, cap, t.kp, t.n, cfg->cos_a, cfg->sin_a, pattern, cfg->edge,
                             t.desc));
  }
  if (slot_of_frame)  // (HOST table: frame i's record goes to record slot_of_frame[i] of o)
    STAGE(sosvo_rgbd_assemble_slots(ctx, cam, t.kp, t.desc, t.n, depth, F, slot_of_frame, cfg->rows, cfg->cols, cap, Fc, o.m, o.d,
                                    o.X, o.b, o.M));
  else
    STAGE(sosvo_rgbd_assemble(ctx, cam, t.kp, t.desc, t.n, depth, F, cfg->rows, cfg->cols, cap, Fc, o.m, o.d, o.X, o.b, o.M));
  return SOSVO_OK;
}

// TrackerRGBDSE3.track_frame (pose_est_tools.py:896-954) for B (reference slot, current slot) pairs of a frame store:
// query = current frame, train = reference frame; central RANSAC (problem i samples with seed + i) + LM.
static int32_t run_rgbd_tracking(sosvo_ctx* ctx, const sosvo_rgbd_batch_cfg* cfg, int B, uint64_t seed, const RgbdStore& s,
                                 const RgbdTrackTmp& b, double* results, const uint64_t* seeds = nullptr) {
  const int Fc = cfg->frame_cap;
  int32_t rc;
  const Gate gate = gate_f2f(*cfg);
  if (cross_f2f(*cfg)) {
    STAGE(mutual_tabs(ctx, b.cur_frame, b.ref_frame, B, b.mutual));
    STAGE(match_mutual(ctx, gate, b.ratio, s.d, s.m, s.M, B, Fc, b.mutual, b.keys));
  } else
    STAGE(match_1nn(ctx, gate, b.ratio, s.d, s.d, s.m, s.m, s.M, s.M, b.cur_frame, b.ref_frame, B, B, Fc, b.keys));
  STAGE(sosvo_sort_matches(ctx, b.keys, s.M, b.cur_frame, B, Fc, b.order));
  STAGE(sosvo_f2f_assemble_central(ctx, cfg->pct_good_matches, cfg->f2f_max_hdiff, s.m, s.X, s.b, s.M, Fc, b.ref_frame,
                                   b.cur_frame, b.keys, b.order, B, Fc, b.f, b.p, b.cq, b.ct, b.cn));
  const int32_t rflags = cfg->flags & (SOSVO_FLAG_EPNP | SOSVO_FLAG_GP3P | SOSVO_FLAG_TWOPT);
  if (seeds)
    STAGE(sosvo_ransac_abs_pose_seeds(ctx, b.f, b.p, nullptr, nullptr, nullptr, 1, rflags, b.cn, B, Fc, cfg->ransac_threshold,
                                      cfg->ransac_max_iter, cfg->ransac_adaptive, seeds, b.T_ransac, b.mask, b.idx, b.n_inl,
                                      b.info, nullptr));
  else
    STAGE(sosvo_ransac_abs_pose(ctx, b.f, b.p, nullptr, nullptr, nullptr, 1, rflags, b.cn, B, Fc, cfg->ransac_threshold,
                                cfg->ransac_max_iter, cfg->ransac_adaptive, seed, b.T_ransac, b.mask, b.idx, b.n_inl, b.info,
                                nullptr));
  SOSVO_HIP(ctx, hipMemcpyAsync(b.T, b.T_ransac, sizeof(double) * 12 * B, hipMemcpyDeviceToDevice, ctx->stream));
  STAGE(sosvo_refine_abs_pose(ctx, b.f, b.p, nullptr, nullptr, nullptr, 1, b.cn, B, Fc, b.idx, b.n_inl, cfg->lm_max_iter, b.T,
                              b.lm_cost, b.lm_iters));
  SOSVO_LAUNCH(ctx, batch_results_kernel, dim3(cdiv(B, 256)), dim3(256), 0, ctx->stream, B, b.T, b.n_inl, b.cn, b.info,
               results);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

int32_t sosvo_rgbd_pair_batch(sosvo_ctx* ctx, const sosvo_rgbd_cam* cam, const sosvo_rgbd_batch_cfg* cfg,
                              const uint8_t* bgr, const float* depth, const uint32_t* mask_bits, const int8_t* pattern,
                              void* workspace, size_t workspace_bytes, double* results) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, cam && cfg && bgr && depth && mask_bits && pattern && workspace && results, "null pointer");
  SOSVO_REQUIRE(ctx, cfg->n_pairs > 0 && cfg->n_pairs <= 8192, "n_pairs out of range (1..8192)");
  SOSVO_REQUIRE(ctx, cfg->kp_cap > 0 && cfg->kp_cap <= 4096 && cfg->frame_cap > 0 && cfg->frame_cap <= 16384,
                "kp_cap / frame_cap out of range");
  SOSVO_REQUIRE(ctx, detector_ok(rgbd_detector(*cfg), cfg->kp_cap), "unknown detector, or ORB with kp_cap > 2048");
  SOSVO_REQUIRE(ctx, rgbd_stereo_flags_ok(*cfg), kRgbdStereoFlags);
  SOSVO_REQUIRE(ctx, ratio_flags_ok(cfg->flags), kBadRatioFlags);
  SOSVO_REQUIRE(ctx, ((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
  const int B = cfg->n_pairs, F = 2 * B;
  const RgbdWorkspace ws = carve_rgbd(*cfg, F, F, workspace);
  SOSVO_REQUIRE(ctx, workspace_bytes >= ws.bytes, "workspace too small (see sosvo_rgbd_pair_batch_workspace)");
  int32_t rc;
  SOSVO_LAUNCH(ctx, pair_index_kernel, dim3(cdiv(B, 256)), dim3(256), 0, ctx->stream, B, ws.tt.ref_frame, ws.tt.cur_frame);
  SOSVO_LAUNCH_CHECK(ctx);
  STAGE(run_rgbd_front_end(ctx, cam, cfg, F, bgr, depth, mask_bits, pattern, ws.fe, ws.store));
  return run_rgbd_tracking(ctx, cfg, B, cfg->seed, ws.store, ws.tt, results);
}

}  // extern "C"

// ---- sequence mode: one body per operation, over a description of the family -------------------------------------
namespace {

template <typename Cfg>
bool seq_shape_ok(const Cfg* cfg, int detector, int32_t window, int32_t slots) {
  return cfg->n_pairs > 0 && cfg->n_pairs <= 8192 && cfg->rows > 0 && cfg->cols > 0 && cfg->kp_cap > 0 && cfg->kp_cap <= 4096 &&
         cfg->frame_cap > 0 && cfg->frame_cap <= 16384 && window >= 1 && window <= 16384 && slots >= window && slots <= 65535 &&
         detector_ok(detector, cfg->kp_cap);
}

// What the input of a front end consists of, besides the configuration and the frame count
struct OmniFrames {
  const sosvo_rig* rig;
  const uint8_t* omni;
  const uint32_t *unwrap_table, *mask_bits;
  const int8_t* pattern;
};
struct RgbdFrames {
  const sosvo_rgbd_cam* cam;
  const uint8_t* bgr;
  const float* depth;
  const uint32_t* mask_bits;
  const int8_t* pattern;
};

// A family of sequence entry points: its configuration, workspace and input types, and its runners.  (`rig` of track():
// the omni rig; the RGB-D tracking calls have none and pass nullptr.)
struct OmniSeq {
  using Cfg = sosvo_batch_cfg;
  using Ws = Workspace;
  using Frames = OmniFrames;
  static constexpr const char* kTooSmall = "workspace too small (see sosvo_sequence_workspace)";
  static bool shape_ok(const Cfg* c, int32_t window, int32_t slots) {
    return c && c->nmask >= 1 && c->nmask <= 32 && !omni_flags_msg(*c) && seq_shape_ok(c, c->detector, window, slots) &&
           (!lk_f2f(*c) || slots <= 32767);  // (the store's images: 2 * slots <= 65535)
  }
  static const char* flags_msg(const Cfg* c) { return omni_flags_msg(*c); }
  static constexpr const char* kBadFrames = SOSVO_TABLE_FRAME_MSG;
  static bool frames_ok(const Cfg* c) { return sosvo_table_frame_ok(c->H, c->W); }  // the front end reads them through the table
  static Ws carve(const Cfg& c, size_t window, size_t slots, void* base) { return ::carve(c, window, slots, base); }
  static StoreFields fields(const FrameStore& s) {
    return {{(char*)s.m_top, (char*)s.m_bot, (char*)s.d_top, (char*)s.d_bot, (char*)s.X, (char*)s.b_top, (char*)s.b_bot},
            {8, 8, 32, 32, 24, 24, 24},
            s.M};
  }
  static int32_t front_end(sosvo_ctx* ctx, const Cfg* cfg, int F, const Frames& in, const Ws& ws, int first_slot,
                           const int32_t* slot_of_frame) {
    return run_front_end(ctx, in.rig, cfg, F, in.omni, in.unwrap_table, in.mask_bits, in.pattern, ws.fe,
                         ws.store.at(first_slot, cfg->frame_cap), nullptr, nullptr, slot_of_frame, &ws, first_slot);
  }
  static int32_t track(sosvo_ctx* ctx, const sosvo_rig* rig, const Cfg* cfg, int B, uint64_t seed, const Ws& ws, double* results,
                       const uint64_t* seeds) {
    return run_tracking(ctx, rig, cfg, B, seed, ws.store, ws.tt, results, seeds, &ws);
  }
  // the images of the copied slots follow their records (SOSVO_FLAG_LK_F2F: the levels the context's settings use)
  static int32_t copy_images(sosvo_ctx* ctx, const CopyPairs& cp, const int32_t* src_list, const int32_t* dst_list, int32_t n,
                             const Ws& ws) {
    if (!ws.img.level[0]) return SOSVO_OK;
    SOSVO_REQUIRE(ctx, sosvo_lk_options_ok(ctx->lk), "LK settings out of range (sosvo_set_lk_options)");
    SOSVO_LAUNCH(ctx, seq_copy_images_kernel, dim3(n, kCopyImageChunks, 2 * ctx->lk.levels), dim3(256), 0, ctx->stream, cp, src_list,
                 dst_list, ws.img);
    SOSVO_LAUNCH_CHECK(ctx);
    return SOSVO_OK;
  }
};
struct RgbdSeq {
  using Cfg = sosvo_rgbd_batch_cfg;
  using Ws = RgbdWorkspace;
  using Frames = RgbdFrames;
  static constexpr const char* kTooSmall = "workspace too small (see sosvo_rgbd_sequence_workspace)";
  static bool shape_ok(const Cfg* c, int32_t window, int32_t slots) {
    return c && rgbd_flags_ok(*c) && seq_shape_ok(c, rgbd_detector(*c), window, slots);
  }
  static const char* flags_msg(const Cfg* c) {
    return !rgbd_stereo_flags_ok(*c) ? kRgbdStereoFlags : ratio_flags_ok(c->flags) ? nullptr : kBadRatioFlags;
  }
  static constexpr const char* kBadFrames = "";
  static bool frames_ok(const Cfg*) { return true; }  // no table: the RGB-D frames are the images
  static Ws carve(const Cfg& c, size_t window, size_t slots, void* base) { return carve_rgbd(c, window, slots, base); }
  static StoreFields fields(const RgbdStore& s) {
    return {{(char*)s.m, (char*)s.d, (char*)s.X, (char*)s.b}, {8, 32, 24, 24}, s.M};
  }
  static int32_t front_end(sosvo_ctx* ctx, const Cfg* cfg, int F, const Frames& in, const Ws& ws, int first_slot,
                           const int32_t* slot_of_frame) {
    return run_rgbd_front_end(ctx, in.cam, cfg, F, in.bgr, in.depth, in.mask_bits, in.pattern, ws.fe,
                              ws.store.at(first_slot, cfg->frame_cap), slot_of_frame);
  }
  static int32_t copy_images(sosvo_ctx*, const CopyPairs&, const int32_t*, const int32_t*, int32_t, const Ws&) { return SOSVO_OK; }
  static int32_t track(sosvo_ctx* ctx, const sosvo_rig*, const Cfg* cfg, int B, uint64_t seed, const Ws& ws, double* results,
                       const uint64_t* seeds) {
    return run_rgbd_tracking(ctx, cfg, B, seed, ws.store, ws.tt, results, seeds);
  }
};

template <typename Fam>
size_t seq_workspace(const typename Fam::Cfg* cfg, int32_t window, int32_t slots) {
  if (!Fam::shape_ok(cfg, window, slots)) return 0;
  return Fam::carve(*cfg, window, slots, nullptr).bytes;
}

// What every sosvo_[rgbd_]sequence_* call checks after its own null check, in this order: the shape, the call's own range
// (range_ok, range_msg), the alignment (aligned == false: ..._frame_counts, which only reads and never asked for it), the
// size.  Errors carry the entry point's name `fn`; on SOSVO_OK `ws` is the carved workspace.
template <typename Fam>
int32_t seq_open(sosvo_ctx* ctx, const char* fn, const typename Fam::Cfg* cfg, int32_t window, int32_t slots, bool range_ok,
                 const char* range_msg, bool aligned, void* workspace, size_t workspace_bytes, typename Fam::Ws& ws) {
  if (cfg && Fam::flags_msg(cfg)) return sosvo_fail(ctx, SOSVO_ERR_ARG, fn, Fam::flags_msg(cfg));  // (a message that says what to fix)
  REQUIRE_FOR(ctx, fn, Fam::shape_ok(cfg, window, slots), "bad sequence configuration (window, slots, capacities)");
  REQUIRE_FOR(ctx, fn, range_ok, range_msg);
  if (aligned) REQUIRE_FOR(ctx, fn, ((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
  ws = Fam::carve(*cfg, window, slots, workspace);
  REQUIRE_FOR(ctx, fn, workspace_bytes >= ws.bytes, Fam::kTooSmall);
  return SOSVO_OK;
}

// ..._front_end (slot_of_frame == nullptr: frame i's record goes to slot first_slot + i) and ..._front_end_slots (HOST table)
template <typename Fam>
int32_t seq_front_end(sosvo_ctx* ctx, const char* fn, const typename Fam::Cfg* cfg, int32_t window, int32_t slots,
                      const typename Fam::Frames& in, int32_t n_frames, int32_t first_slot, const int32_t* slot_of_frame,
                      void* workspace, size_t workspace_bytes) {
  typename Fam::Ws ws;
  int32_t rc;
  const bool fits = slot_of_frame ? n_frames <= slots : first_slot >= 0 && first_slot + n_frames <= slots;
  REQUIRE_FOR(ctx, fn, Fam::frames_ok(cfg), Fam::kBadFrames);  // (first: a frame size, not a matter of the workspace)
  STAGE(seq_open<Fam>(ctx, fn, cfg, window, slots, n_frames >= 0 && n_frames <= window && fits,
                      "frames do not fit the window / the store", true, workspace, workspace_bytes, ws));
  if (slot_of_frame) STAGE(check_slot_table(ctx, fn, slot_of_frame, n_frames, slots));
  if (n_frames == 0) return SOSVO_OK;
  return Fam::front_end(ctx, cfg, n_frames, in, ws, slot_of_frame ? 0 : first_slot, slot_of_frame);
}

// ..._track (seed_host == nullptr: pair i samples with seed + i) and ..._track_seeds (HOST list, `seed` unused): the slot
// pairs reach the device, then the family's tracking.  The setup kernel is launched whenever it has something to write:
// slot pairs that travel as its arguments, or the rig's cam_off / cam_rot (every omni call).
template <typename Fam>
int32_t seq_track(sosvo_ctx* ctx, const char* fn, const sosvo_rig* rig, const typename Fam::Cfg* cfg, int32_t window,
                  int32_t slots, const int32_t* ref_slot, const int32_t* cur_slot, uint64_t seed, const uint64_t* seed_host,
                  int32_t n_pairs, void* workspace, size_t workspace_bytes, double* results) {
  typename Fam::Ws ws;
  int32_t rc;
  STAGE(seq_open<Fam>(ctx, fn, cfg, window, slots, n_pairs >= 0 && n_pairs <= cfg->n_pairs, "more slot pairs than cfg->n_pairs",
                      true, workspace, workspace_bytes, ws));
  if (n_pairs == 0) return SOSVO_OK;
  SlotPairs sp;
  PairSeeds ps;
  STAGE(upload_slot_pairs(ctx, fn, ref_slot, cur_slot, seed_host, n_pairs, slots, ws.tt, sp, ps));
  uint64_t* seeds = seed_host ? pair_seeds(ws.tt) : nullptr;
  if (rig || n_pairs <= kSeqArgPairs) {
    SOSVO_LAUNCH(ctx, seq_setup_kernel, dim3(1), dim3(64), 0, ctx->stream, n_pairs > kSeqArgPairs ? 0 : n_pairs, sp, ps,
                 rig ? foci_of(rig) : Foci{}, ws.tt.ref_frame, ws.tt.cur_frame, seeds, ws.tt.cam_off, ws.tt.cam_rot);
    SOSVO_LAUNCH_CHECK(ctx);
  }
  return Fam::track(ctx, rig, cfg, n_pairs, seed_host ? 0 : seed, ws, results, seeds);
}

// n (source, destination) pairs of the store `st` in one launch: in `cp` up to kSeqArgPairs, in the device lists beyond
int32_t launch_copy(sosvo_ctx* ctx, const CopyPairs& cp, const int32_t* src_list, const int32_t* dst_list, int32_t n, int Fc,
                    const StoreFields& st) {
  SOSVO_LAUNCH(ctx, seq_copy_slots_kernel, dim3(n, kCopyChunks), dim3(256), 0, ctx->stream, cp, src_list, dst_list, Fc, st);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

template <typename Fam>
int32_t seq_copy_slot(sosvo_ctx* ctx, const char* fn, const typename Fam::Cfg* cfg, int32_t window, int32_t slots, int32_t src,
                      int32_t dst, void* workspace, size_t workspace_bytes) {
  typename Fam::Ws ws;
  int32_t rc;
  STAGE(seq_open<Fam>(ctx, fn, cfg, window, slots, src >= 0 && src < slots && dst >= 0 && dst < slots, "slot out of range", true,
                      workspace, workspace_bytes, ws));
  if (src == dst) return SOSVO_OK;
  CopyPairs cp{};
  cp.src[0] = src;
  cp.dst[0] = dst;
  STAGE(launch_copy(ctx, cp, nullptr, nullptr, 1, cfg->frame_cap, Fam::fields(ws.store)));
  return Fam::copy_images(ctx, cp, nullptr, nullptr, 1, ws);
}

template <typename Fam>
int32_t seq_copy_slots(sosvo_ctx* ctx, const char* fn, const typename Fam::Cfg* cfg, int32_t window, int32_t slots,
                       const int32_t* src, const int32_t* dst, int32_t n, void* workspace, size_t workspace_bytes) {
  typename Fam::Ws ws;
  int32_t rc;
  STAGE(seq_open<Fam>(ctx, fn, cfg, window, slots, n >= 0 && n <= cfg->n_pairs, "more copies than cfg->n_pairs", true, workspace,
                      workspace_bytes, ws));
  CopyPairs cp;
  STAGE(check_copy_lists(ctx, fn, src, dst, n, slots, cp));
  if (n == 0) return SOSVO_OK;
  const bool copied = n > kSeqArgPairs;  // (the lists go where a tracking call keeps its slot pairs)
  if (copied) {
    SOSVO_HIP(ctx, hipMemcpyAsync(ws.tt.ref_frame, src, sizeof(int32_t) * n, hipMemcpyHostToDevice, ctx->stream));
    SOSVO_HIP(ctx, hipMemcpyAsync(ws.tt.cur_frame, dst, sizeof(int32_t) * n, hipMemcpyHostToDevice, ctx->stream));
  }
  STAGE(launch_copy(ctx, cp, copied ? ws.tt.ref_frame : nullptr, copied ? ws.tt.cur_frame : nullptr, n, cfg->frame_cap,
                    Fam::fields(ws.store)));
  return Fam::copy_images(ctx, cp, copied ? ws.tt.ref_frame : nullptr, copied ? ws.tt.cur_frame : nullptr, n, ws);
}

template <typename Fam>
int32_t seq_frame_counts(sosvo_ctx* ctx, const char* fn, const typename Fam::Cfg* cfg, int32_t window, int32_t slots,
                         int32_t first_slot, int32_t n, void* workspace, size_t workspace_bytes, int32_t* counts_host) {
  typename Fam::Ws ws;
  int32_t rc;
  STAGE(seq_open<Fam>(ctx, fn, cfg, window, slots, first_slot >= 0 && n >= 0 && first_slot + n <= slots, "slots out of range",
                      false, workspace, workspace_bytes, ws));
  if (n == 0) return SOSVO_OK;
  SOSVO_HIP(ctx, hipMemcpyAsync(counts_host, ws.store.M + first_slot, sizeof(int32_t) * n, hipMemcpyDeviceToHost, ctx->stream));
  SOSVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SOSVO_OK;
}

}  // namespace

extern "C" {

size_t sosvo_sequence_workspace(const sosvo_batch_cfg* cfg, int32_t window, int32_t slots) {
  return seq_workspace<OmniSeq>(cfg, window, slots);
}

int32_t sosvo_sequence_front_end(sosvo_ctx* ctx, const sosvo_rig* rig, const sosvo_batch_cfg* cfg, int32_t window, int32_t slots,
                                 const uint8_t* omni, int32_t n_frames, int32_t first_slot, const uint32_t* unwrap_table,
                                 const uint32_t* mask_bits, const int8_t* pattern, void* workspace, size_t workspace_bytes) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, rig && cfg && omni && unwrap_table && mask_bits && pattern && workspace, "null pointer");
  return seq_front_end<OmniSeq>(ctx, __func__, cfg, window, slots, {rig, omni, unwrap_table, mask_bits, pattern}, n_frames,
                                first_slot, nullptr, workspace, workspace_bytes);
}

int32_t sosvo_sequence_front_end_slots(sosvo_ctx* ctx, const sosvo_rig* rig, const sosvo_batch_cfg* cfg, int32_t window,
                                       int32_t slots, const uint8_t* omni, int32_t n_frames, const int32_t* slot_of_frame,
                                       const uint32_t* unwrap_table, const uint32_t* mask_bits, const int8_t* pattern,
                                       void* workspace, size_t workspace_bytes) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, rig && cfg && omni && slot_of_frame && unwrap_table && mask_bits && pattern && workspace, "null pointer");
  return seq_front_end<OmniSeq>(ctx, __func__, cfg, window, slots, {rig, omni, unwrap_table, mask_bits, pattern}, n_frames, 0,
                                slot_of_frame, workspace, workspace_bytes);
}

int32_t sosvo_sequence_track(sosvo_ctx* ctx, const sosvo_rig* rig, const sosvo_batch_cfg* cfg, int32_t window, int32_t slots,
                             const int32_t* ref_slot, const int32_t* cur_slot, int32_t n_pairs, uint64_t seed, void* workspace,
                             size_t workspace_bytes, double* results) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, rig && cfg && ref_slot && cur_slot && workspace && results, "null pointer");
  return seq_track<OmniSeq>(ctx, __func__, rig, cfg, window, slots, ref_slot, cur_slot, seed, nullptr, n_pairs, workspace,
                            workspace_bytes, results);
}

int32_t sosvo_sequence_track_seeds(sosvo_ctx* ctx, const sosvo_rig* rig, const sosvo_batch_cfg* cfg, int32_t window,
                                   int32_t slots, const int32_t* ref_slot, const int32_t* cur_slot, const uint64_t* seed,
                                   int32_t n_pairs, void* workspace, size_t workspace_bytes, double* results) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, rig && cfg && ref_slot && cur_slot && seed && workspace && results, "null pointer");
  return seq_track<OmniSeq>(ctx, __func__, rig, cfg, window, slots, ref_slot, cur_slot, 0, seed, n_pairs, workspace,
                            workspace_bytes, results);
}

int32_t sosvo_sequence_copy_slot(sosvo_ctx* ctx, const sosvo_batch_cfg* cfg, int32_t window, int32_t slots, int32_t src_slot,
                                 int32_t dst_slot, void* workspace, size_t workspace_bytes) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, cfg && workspace, "null pointer");
  return seq_copy_slot<OmniSeq>(ctx, __func__, cfg, window, slots, src_slot, dst_slot, workspace, workspace_bytes);
}

int32_t sosvo_sequence_copy_slots(sosvo_ctx* ctx, const sosvo_batch_cfg* cfg, int32_t window, int32_t slots,
                                  const int32_t* src_slot, const int32_t* dst_slot, int32_t n_copies, void* workspace,
                                  size_t workspace_bytes) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, cfg && src_slot && dst_slot && workspace, "null pointer");
  return seq_copy_slots<OmniSeq>(ctx, __func__, cfg, window, slots, src_slot, dst_slot, n_copies, workspace, workspace_bytes);
}

int32_t sosvo_sequence_frame_counts(sosvo_ctx* ctx, const sosvo_batch_cfg* cfg, int32_t window, int32_t slots, int32_t first_slot,
                                    int32_t n, void* workspace, size_t workspace_bytes, int32_t* counts_host) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, cfg && workspace && counts_host, "null pointer");
  return seq_frame_counts<OmniSeq>(ctx, __func__, cfg, window, slots, first_slot, n, workspace, workspace_bytes, counts_host);
}

size_t sosvo_rgbd_sequence_workspace(const sosvo_rgbd_batch_cfg* cfg, int32_t window, int32_t slots) {
  return seq_workspace<RgbdSeq>(cfg, window, slots);
}

int32_t sosvo_rgbd_sequence_front_end(sosvo_ctx* ctx, const sosvo_rgbd_cam* cam, const sosvo_rgbd_batch_cfg* cfg, int32_t window,
                                      int32_t slots, const uint8_t* bgr, const float* depth, int32_t n_frames, int32_t first_slot,
                                      const uint32_t* mask_bits, const int8_t* pattern, void* workspace, size_t workspace_bytes) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, cam && cfg && bgr && depth && mask_bits && pattern && workspace, "null pointer");
  return seq_front_end<RgbdSeq>(ctx, __func__, cfg, window, slots, {cam, bgr, depth, mask_bits, pattern}, n_frames, first_slot,
                                nullptr, workspace, workspace_bytes);
}

int32_t sosvo_rgbd_sequence_front_end_slots(sosvo_ctx* ctx, const sosvo_rgbd_cam* cam, const sosvo_rgbd_batch_cfg* cfg,
                                            int32_t window, int32_t slots, const uint8_t* bgr, const float* depth,
                                            int32_t n_frames, const int32_t* slot_of_frame, const uint32_t* mask_bits,
                                            const int8_t* pattern, void* workspace, size_t workspace_bytes) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, cam && cfg && bgr && depth && slot_of_frame && mask_bits && pattern && workspace, "null pointer");
  return seq_front_end<RgbdSeq>(ctx, __func__, cfg, window, slots, {cam, bgr, depth, mask_bits, pattern}, n_frames, 0,
                                slot_of_frame, workspace, workspace_bytes);
}

int32_t sosvo_rgbd_sequence_track(sosvo_ctx* ctx, const sosvo_rgbd_batch_cfg* cfg, int32_t window, int32_t slots,
                                  const int32_t* ref_slot, const int32_t* cur_slot, int32_t n_pairs, uint64_t seed, void* workspace,
                                  size_t workspace_bytes, double* results) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, cfg && ref_slot && cur_slot && workspace && results, "null pointer");
  return seq_track<RgbdSeq>(ctx, __func__, nullptr, cfg, window, slots, ref_slot, cur_slot, seed, nullptr, n_pairs, workspace,
                            workspace_bytes, results);
}

int32_t sosvo_rgbd_sequence_track_seeds(sosvo_ctx* ctx, const sosvo_rgbd_batch_cfg* cfg, int32_t window, int32_t slots,
                                        const int32_t* ref_slot, const int32_t* cur_slot, const uint64_t* seed, int32_t n_pairs,
                                        void* workspace, size_t workspace_bytes, double* results) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, cfg && ref_slot && cur_slot && seed && workspace && results, "null pointer");
  return seq_track<RgbdSeq>(ctx, __func__, nullptr, cfg, window, slots, ref_slot, cur_slot, 0, seed, n_pairs, workspace,
                            workspace_bytes, results);
}

int32_t sosvo_rgbd_sequence_copy_slot(sosvo_ctx* ctx, const sosvo_rgbd_batch_cfg* cfg, int32_t window, int32_t slots,
                                      int32_t src_slot, int32_t dst_slot, void* workspace, size_t workspace_bytes) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, cfg && workspace, "null pointer");
  return seq_copy_slot<RgbdSeq>(ctx, __func__, cfg, window, slots, src_slot, dst_slot, workspace, workspace_bytes);
}

int32_t sosvo_rgbd_sequence_copy_slots(sosvo_ctx* ctx, const sosvo_rgbd_batch_cfg* cfg, int32_t window, int32_t slots,
                                       const int32_t* src_slot, const int32_t* dst_slot, int32_t n_copies, void* workspace,
                                       size_t workspace_bytes) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, cfg && src_slot && dst_slot && workspace, "null pointer");
  return seq_copy_slots<RgbdSeq>(ctx, __func__, cfg, window, slots, src_slot, dst_slot, n_copies, workspace, workspace_bytes);
}

int32_t sosvo_rgbd_sequence_frame_counts(sosvo_ctx* ctx, const sosvo_rgbd_batch_cfg* cfg, int32_t window, int32_t slots,
                                         int32_t first_slot, int32_t n, void* workspace, size_t workspace_bytes,
                                         int32_t* counts_host) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, cfg && workspace && counts_host, "null pointer");
  return seq_frame_counts<RgbdSeq>(ctx, __func__, cfg, window, slots, first_slot, n, workspace, workspace_bytes, counts_host);
}

}  // extern "C"
