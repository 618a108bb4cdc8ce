// Geometry stages of the hot path: pano pixel -> bearing (a7, a8), midpoint triangulation (a9),
// range filter (a10), RGB-D back-projection (a12), and the two fused "assemble" kernels that
// replace the Python list/fancy-indexing glue between matching and RANSAC:
//   stereo_assemble: OmniStereoModel.match_features_panoramic_top_bottom (camera_models.py:3027-3101)
//                    + StereoPanoramicFrame.establish_stereo_correspondences (pose_est_tools.py:339-397)
//   f2f_assemble:    match_features_frame_to_frame (pose_est_tools.py:211-269)
//                    + the stacking of TrackerStereoSE3.track_frame (pose_est_tools.py:752-778)
// Both keep the reference's ordering (bucket order, then ascending distance with ties in query
// order; top view before bottom view) by stable compaction: wave ballot prefix + a running base.
// All are HBM/latency-bound elementwise work: one lane per correspondence, coalesced rows.
#include "common.h"
#include "geom_core.h"

namespace {

constexpr int kThreads = 256;

__global__ void pano_to_bearing_kernel(const double* __restrict__ uv, int n, double cols, double rows, double px,
                                       double hmax, double* __restrict__ az, double* __restrict__ el,
                                       double* __restrict__ b3) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double pano[4] = {cols, rows, px, hmax};
  double a, e, b[3];
  sv_pano_angles(uv[2 * i], uv[2 * i + 1], pano, &a, &e);
  sv_bearing(a, e, b);
  if (az) az[i] = a;
  if (el) el[i] = e;
  if (b3) {
    b3[3 * i] = b[0];
    b3[3 * i + 1] = b[1];
    b3[3 * i + 2] = b[2];
  }
}

struct F3x2 {
  double F1[3], F2[3];
};

__global__ void triangulate_kernel(const double* __restrict__ az1, const double* __restrict__ el1,
                                   const double* __restrict__ az2, const double* __restrict__ el2, int n, F3x2 foci,
                                   double* __restrict__ X) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double x[3];
  sv_triangulate(az1[i], el1[i], az2[i], el2[i], foci.F1, foci.F2, x);
  X[3 * i] = x[0];
  X[3 * i + 1] = x[1];
  X[3 * i + 2] = x[2];
}

struct Rt12 {
  double t[3], R[9];
};

__global__ void triangulate2_kernel(const double* __restrict__ b1, const double* __restrict__ b2, int n, Rt12 rt,
                                    double* __restrict__ X) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double f1[3] = {b1[3 * i], b1[3 * i + 1], b1[3 * i + 2]}, f2[3] = {b2[3 * i], b2[3 * i + 1], b2[3 * i + 2]};
  double x[3];
  sv_triangulate2(f1, f2, rt.t, rt.R, x);
  X[3 * i] = x[0];
  X[3 * i + 1] = x[1];
  X[3 * i + 2] = x[2];
}

__global__ void range_filter_kernel(const double* __restrict__ X, int n, double min_range, double max_range,
                                    uint8_t* __restrict__ ok) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x[3] = {X[3 * i], X[3 * i + 1], X[3 * i + 2]};
  ok[i] = sv_range_ok(x, min_range, max_range) ? 1 : 0;
}

struct Intr {
  double fx, fy, cx, cy, fl;
};

// camera_models.py:781-799 (radial depth -> Z; focal_length * depth stays float32), :845-860, :203-212
__global__ void rgbd_backproject_kernel(const float* __restrict__ depth, int rows, int cols,
                                        const int32_t* __restrict__ u, const int32_t* __restrict__ v, int n, Intr k,
                                        int depth_is_Z, double* __restrict__ xyz, double* __restrict__ bearing) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int ui = min(max(u[i], 0), cols - 1), vi = min(max(v[i], 0), rows - 1);
  const float dv = depth[(size_t)vi * cols + ui];
  double d = (double)dv;
  if (!depth_is_Z) {
    const double xi = (k.fl / k.fx) * ((double)ui - k.cx), yi = (k.fl / k.fy) * ((double)vi - k.cy), zi = k.fl;
    const float fd = (float)k.fl * dv;
    d = (double)fd / sqrt(xi * xi + yi * yi + zi * zi);
  }
  const double Z = (d != 0.0) ? d : sv_nan();
  const double X = ((double)ui - k.cx) * Z / k.fx, Y = ((double)vi - k.cy) * Z / k.fy;
  xyz[3 * i] = X;
  xyz[3 * i + 1] = Y;
  xyz[3 * i + 2] = Z;
  const double nrm = sqrt(X * X + Y * Y + Z * Z);
  bearing[3 * i] = X / nrm;
  bearing[3 * i + 1] = Y / nrm;
  bearing[3 * i + 2] = Z / nrm;
}

// The record of input frame `fr` (one workgroup) written at record `slot` of the outputs.
__device__ __forceinline__ void stereo_assemble_frame(
    const int fr, const int slot, const sosvo_rig& rig, const float* __restrict__ kp_top, const float* __restrict__ kp_bot,
    const uint4* __restrict__ desc_top, const uint4* __restrict__ desc_bot, const int32_t* __restrict__ n_top,
    const int32_t* __restrict__ n_bot, const uint32_t* __restrict__ keys, const int32_t* __restrict__ order, int nmask,
    int cap, int out_cap, float* __restrict__ m_top, float* __restrict__ m_bot, uint4* __restrict__ d_top,
    uint4* __restrict__ d_bot, double* __restrict__ X, double* __restrict__ b_top, double* __restrict__ b_bot,
    int32_t* __restrict__ M, int32_t* __restrict__ n_cand) {
  SOSVO_LATENCY_BOUND_PRIO();
  __shared__ int wave_off[kThreads / 64 + 1];
  __shared__ int s_running, s_cand;
  const int tid = threadIdx.x;
  if (tid == 0) s_running = s_cand = 0;
  __syncthreads();
  // len(matches) is the number of keys that are not SOSVO_KEY_NONE: every query's when the train set is not empty, the
  // mutual matches alone after sosvo_cross_check_matches (the sort put them first).  With pct_good_matches == 1 (the
  // trackers' setting) every one of them is a candidate, so the ranks are walked to nq and a NONE key is no match; any
  // other fraction needs the count before the walk.
  const bool take_all = rig.pct_good_matches == 1.0;
  for (int m = 0; m < nmask; ++m) {
    const int p = fr * nmask + m;
    const int nq = min(n_bot[p], cap), nt = min(n_top[p], cap);
    if (nq == 0 || nt == 0) continue;                                 // camera_models.py:3039
    const size_t pb = (size_t)p * cap;
    const int kept = take_all ? nq : sosvo_block_count_matches(keys + pb, nq, tid, kThreads);
    const int good = (int)(rig.pct_good_matches * (double)kept);      // camera_models.py:3045
    for (int r0 = 0; r0 < good; r0 += kThreads) {
      const int r = r0 + tid;
      bool valid = false, matched = false;
      int q = 0, t = 0;
      double xyz[3], bt[3], bb[3];
      float ut = 0, vt = 0, ub = 0, vb = 0;
      if (r < good) {
        q = order[pb + r];                                            // query = bottom (:3042)
        const uint32_t key = keys[pb + q];
        matched = key != SOSVO_KEY_NONE;
        t = matched ? (int)(key & SOSVO_KEY_IDX_MASK) : 0;            // train = top
      }
      if (n_cand) {                                                   // candidates = matches among the first `good` ranks
        const unsigned long long bal = __ballot(matched);
        if ((tid & 63) == 0 && bal) atomicAdd(&s_cand, __popcll(bal));
      }
      if (matched) {
        ut = kp_top[2 * (pb + t)];
        vt = kp_top[2 * (pb + t) + 1];
        ub = kp_bot[2 * (pb + q)];
        vb = kp_bot[2 * (pb + q) + 1];
        valid = sv_pixel_gate((double)ut, (double)vt, (double)ub, (double)vb, rig.stereo_min_disp, rig.stereo_max_hdiff);
        double az1, el1, az2, el2;
        sv_pano_angles((double)ut, (double)vt, rig.pano_top, &az1, &el1);
        sv_pano_angles((double)ub, (double)vb, rig.pano_bot, &az2, &el2);
        sv_bearing(az1, el1, bt);
        sv_bearing(az2, el2, bb);
        sv_triangulate(az1, el1, az2, el2, rig.F_top, rig.F_bot, xyz);
        valid = valid && sv_range_ok(xyz, rig.min_range, rig.max_range);
      }
      const int pos = sosvo_block_compact_pos<kThreads / 64>(valid, wave_off, &s_running, tid);
      if (valid && pos < out_cap) {
        const size_t o = (size_t)slot * out_cap + pos;
        m_top[2 * o] = ut;
        m_top[2 * o + 1] = vt;
        m_bot[2 * o] = ub;
        m_bot[2 * o + 1] = vb;
        d_top[2 * o] = desc_top[2 * (pb + t)];
        d_top[2 * o + 1] = desc_top[2 * (pb + t) + 1];
        d_bot[2 * o] = desc_bot[2 * (pb + q)];
        d_bot[2 * o + 1] = desc_bot[2 * (pb + q) + 1];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          X[3 * o + k] = xyz[k];
          b_top[3 * o + k] = bt[k];
          b_bot[3 * o + k] = bb[k];
        }
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    M[slot] = min(s_running, out_cap);
    if (n_cand) n_cand[fr] = s_cand;
  }
}

// frame blockIdx.x -> record blockIdx.x
__global__ __launch_bounds__(kThreads) void stereo_assemble_kernel(
    sosvo_rig rig, const float* __restrict__ kp_top, const float* __restrict__ kp_bot,
    const uint4* __restrict__ desc_top, const uint4* __restrict__ desc_bot, const int32_t* __restrict__ n_top,
    const int32_t* __restrict__ n_bot, const uint32_t* __restrict__ keys, const int32_t* __restrict__ order, int nmask,
    int cap, int out_cap, float* __restrict__ m_top, float* __restrict__ m_bot, uint4* __restrict__ d_top,
    uint4* __restrict__ d_bot, double* __restrict__ X, double* __restrict__ b_top, double* __restrict__ b_bot,
    int32_t* __restrict__ M, int32_t* __restrict__ n_cand) {
  stereo_assemble_frame(blockIdx.x, blockIdx.x, rig, kp_top, kp_bot, desc_top, desc_bot, n_top, n_bot, keys, order, nmask, cap,
                        out_cap, m_top, m_bot, d_top, d_bot, X, b_top, b_bot, M, n_cand);
}

// frame frame0 + blockIdx.x -> record tab.slot[blockIdx.x] (sosvo_sequence_front_end_slots: the frames of one call belong
// to several sequences whose store slots are not one range).  The table travels as a kernel argument: no copy per call.
__global__ __launch_bounds__(kThreads) void stereo_assemble_slots_kernel(
    sosvo_rig rig, sosvo_slot_table tab, int frame0, const float* __restrict__ kp_top, const float* __restrict__ kp_bot,
    const uint4* __restrict__ desc_top, const uint4* __restrict__ desc_bot, const int32_t* __restrict__ n_top,
    const int32_t* __restrict__ n_bot, const uint32_t* __restrict__ keys, const int32_t* __restrict__ order, int nmask,
    int cap, int out_cap, float* __restrict__ m_top, float* __restrict__ m_bot, uint4* __restrict__ d_top,
    uint4* __restrict__ d_bot, double* __restrict__ X, double* __restrict__ b_top, double* __restrict__ b_bot,
    int32_t* __restrict__ M, int32_t* __restrict__ n_cand) {
  stereo_assemble_frame(frame0 + (int)blockIdx.x, tab.slot[blockIdx.x], rig, kp_top, kp_bot, desc_top, desc_bot, n_top, n_bot,
                        keys, order, nmask, cap, out_cap, m_top, m_bot, d_top, d_bot, X, b_top, b_bot, M, n_cand);
}

// The CYCLIC frame-to-frame |du| gate: a panorama's column W is column 0 again, so a pair passes iff
// d <= max_du or W - d <= max_du, d = |a - b| in double from the float32 values.  Both comparisons are exact (differences of
// float32 coordinates below 16384 and W - d are doubles), and the switch is sv_pixel_gate's: on for max_du > 0.
__device__ __forceinline__ bool f2f_du_gate_cyclic(double ua, double ub, double max_du, double W) {
  if (!(max_du > 0)) return true;
  const double d = fabs(ua - ub);
  return d <= max_du || W - d <= max_du;
}

// (CYC: the gate above with the view's period rig.pano_top[0] / rig.pano_bot[0]; nothing else differs)
template <bool CYC>
__device__ __forceinline__ void f2f_assemble_body(
    const sosvo_rig& rig, const float* __restrict__ m_top, const float* __restrict__ m_bot, const double* __restrict__ X,
    const double* __restrict__ b_top, const double* __restrict__ b_bot, const int32_t* __restrict__ M, int frame_cap,
    const int32_t* __restrict__ ref_frame, const int32_t* __restrict__ cur_frame,
    const uint32_t* __restrict__ keys_top, const int32_t* __restrict__ order_top,
    const uint32_t* __restrict__ keys_bot, const int32_t* __restrict__ order_bot, int corr_cap,
    double* __restrict__ f, double* __restrict__ p, int32_t* __restrict__ cam, int32_t* __restrict__ corr_q,
    int32_t* __restrict__ corr_t, int32_t* __restrict__ n, int32_t* __restrict__ n_topview) {
  SOSVO_LATENCY_BOUND_PRIO();
  __shared__ int wave_off[kThreads / 64 + 1];
  __shared__ int s_running;
  const int tid = threadIdx.x, pr = blockIdx.x;
  if (tid == 0) s_running = 0;
  __syncthreads();
  const int fr_ref = ref_frame[pr], fr_cur = cur_frame[pr];
  const int nq = min(M[fr_cur], frame_cap), nt = min(M[fr_ref], frame_cap);
  const bool take_all = rig.pct_good_matches == 1.0;
  const size_t kb = (size_t)pr * frame_cap;
  for (int view = 0; view < 2; ++view) {
    const uint32_t* keys = view == 0 ? keys_top : keys_bot;
    // len(matches) = the keys that are not SOSVO_KEY_NONE, as in stereo_assemble_frame: walked to nq when every match is
    // taken, counted first otherwise
    const int kept = nt == 0 ? 0 : take_all ? nq : sosvo_block_count_matches(keys + kb, nq, tid, kThreads);
    const int good = (int)(rig.pct_good_matches * (double)kept);  // pose_est_tools.py:225
    const int32_t* order = view == 0 ? order_top : order_bot;
    const float* mm = view == 0 ? m_top : m_bot;
    const double* bb = view == 0 ? b_top : b_bot;
    for (int r0 = 0; r0 < good; r0 += kThreads) {
      const int r = r0 + tid;
      bool valid = false;
      int q = 0, t = 0;
      if (r < good) {
        q = order[kb + r];                                  // query = current frame (:215)
        const uint32_t key = keys[kb + q];
        valid = key != SOSVO_KEY_NONE;
        t = valid ? (int)(key & SOSVO_KEY_IDX_MASK) : 0;    // train = reference (key)frame
        if (valid && rig.f2f_max_hdiff >= 0) {              // :245-247, gate inside common_cv.py:177
          const double u_train = (double)mm[2 * ((size_t)fr_ref * frame_cap + t)];
          const double u_query = (double)mm[2 * ((size_t)fr_cur * frame_cap + q)];
          if constexpr (CYC)
            valid = f2f_du_gate_cyclic(u_train, u_query, rig.f2f_max_hdiff, view == 0 ? rig.pano_top[0] : rig.pano_bot[0]);
          else
            valid = sv_pixel_gate(u_train, 0.0, u_query, 0.0, -1.0, rig.f2f_max_hdiff);
        }
      }
      const int pos = sosvo_block_compact_pos<kThreads / 64>(valid, wave_off, &s_running, tid);
      if (valid && pos < corr_cap) {
        const size_t o = (size_t)pr * corr_cap + pos;
        const size_t qrow = (size_t)fr_cur * frame_cap + q, trow = (size_t)fr_ref * frame_cap + t;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          f[3 * o + k] = bb[3 * qrow + k];                  // bearings of the CURRENT frame (:752,:755)
          p[3 * o + k] = X[3 * trow + k];                   // 3-D points of the REFERENCE frame (:753,:756)
        }
        cam[o] = view;
        corr_q[o] = q;
        corr_t[o] = t;
      }
    }
    __syncthreads();
    if (view == 0 && tid == 0 && n_topview) n_topview[pr] = min(s_running, corr_cap);
  }
  __syncthreads();
  if (tid == 0) n[pr] = min(s_running, corr_cap);
}
__global__ __launch_bounds__(kThreads) void f2f_assemble_kernel(
    sosvo_rig rig, const float* __restrict__ m_top, const float* __restrict__ m_bot, const double* __restrict__ X,
    const double* __restrict__ b_top, const double* __restrict__ b_bot, const int32_t* __restrict__ M, int frame_cap,
    const int32_t* __restrict__ ref_frame, const int32_t* __restrict__ cur_frame,
    const uint32_t* __restrict__ keys_top, const int32_t* __restrict__ order_top,
    const uint32_t* __restrict__ keys_bot, const int32_t* __restrict__ order_bot, int corr_cap,
    double* __restrict__ f, double* __restrict__ p, int32_t* __restrict__ cam, int32_t* __restrict__ corr_q,
    int32_t* __restrict__ corr_t, int32_t* __restrict__ n, int32_t* __restrict__ n_topview) {
  f2f_assemble_body<false>(rig, m_top, m_bot, X, b_top, b_bot, M, frame_cap, ref_frame, cur_frame, keys_top, order_top, keys_bot, order_bot, corr_cap, f,
                           p, cam, corr_q, corr_t, n, n_topview);
}
__global__ __launch_bounds__(kThreads) void f2f_assemble_cyclic_kernel(
    sosvo_rig rig, const float* __restrict__ m_top, const float* __restrict__ m_bot, const double* __restrict__ X,
    const double* __restrict__ b_top, const double* __restrict__ b_bot, const int32_t* __restrict__ M, int frame_cap,
    const int32_t* __restrict__ ref_frame, const int32_t* __restrict__ cur_frame,
    const uint32_t* __restrict__ keys_top, const int32_t* __restrict__ order_top,
    const uint32_t* __restrict__ keys_bot, const int32_t* __restrict__ order_bot, int corr_cap,
    double* __restrict__ f, double* __restrict__ p, int32_t* __restrict__ cam, int32_t* __restrict__ corr_q,
    int32_t* __restrict__ corr_t, int32_t* __restrict__ n, int32_t* __restrict__ n_topview) {
  f2f_assemble_body<true>(rig, m_top, m_bot, X, b_top, b_bot, M, frame_cap, ref_frame, cur_frame, keys_top, order_top, keys_bot, order_bot, corr_cap, f,
                           p, cam, corr_q, corr_t, n, n_topview);
}

// f2f_assemble_kernel for tracked points: the correspondences of pair pr are the reference frame's points whose track
// succeeded, in point order; the bearing of the tracked pixel is computed here, as stereo_assemble_frame computes its own.
template <bool CYC>
__device__ __forceinline__ void f2f_assemble_tracked_body(
    const sosvo_rig& rig, const float* __restrict__ m_top, const float* __restrict__ m_bot, const double* __restrict__ X,
    const int32_t* __restrict__ M, int frame_cap, const int32_t* __restrict__ ref_frame, const float* __restrict__ trk_top,
    const float* __restrict__ trk_bot, const uint8_t* __restrict__ st_top, const uint8_t* __restrict__ st_bot, int corr_cap,
    double* __restrict__ f, double* __restrict__ p, int32_t* __restrict__ cam, int32_t* __restrict__ corr_q,
    int32_t* __restrict__ corr_t, int32_t* __restrict__ n, int32_t* __restrict__ n_topview) {
  SOSVO_LATENCY_BOUND_PRIO();
  __shared__ int wave_off[kThreads / 64 + 1];
  __shared__ int s_running;
  const int tid = threadIdx.x, pr = blockIdx.x;
  if (tid == 0) s_running = 0;
  __syncthreads();
  const int fr_ref = ref_frame[pr];
  const int nt = min(max(M[fr_ref], 0), frame_cap);
  const size_t kb = (size_t)pr * frame_cap, rb = (size_t)fr_ref * frame_cap;
  for (int view = 0; view < 2; ++view) {
    const float* mm = view == 0 ? m_top : m_bot;
    const float* trk = view == 0 ? trk_top : trk_bot;
    const uint8_t* st = view == 0 ? st_top : st_bot;
    const double* pano = view == 0 ? rig.pano_top : rig.pano_bot;
    for (int t0 = 0; t0 < nt; t0 += kThreads) {
      const int t = t0 + tid;
      bool valid = false;
      double b[3] = {0.0, 0.0, 0.0};
      if (t < nt && st[kb + t] != 0) {
        const double u = (double)trk[2 * (kb + t)], v = (double)trk[2 * (kb + t) + 1];
        valid = true;
        if (rig.f2f_max_hdiff >= 0) {
          if constexpr (CYC)
            valid = f2f_du_gate_cyclic((double)mm[2 * (rb + t)], u, rig.f2f_max_hdiff, pano[0]);
          else
            valid = sv_pixel_gate((double)mm[2 * (rb + t)], 0.0, u, 0.0, -1.0, rig.f2f_max_hdiff);
        }
        double az, el;
        sv_pano_angles(u, v, pano, &az, &el);
        sv_bearing(az, el, b);
      }
      const int pos = sosvo_block_compact_pos<kThreads / 64>(valid, wave_off, &s_running, tid);
      if (valid && pos < corr_cap) {
        const size_t o = (size_t)pr * corr_cap + pos;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          f[3 * o + k] = b[k];
          p[3 * o + k] = X[3 * (rb + t) + k];
        }
        cam[o] = view;
        corr_q[o] = -1;
        corr_t[o] = t;
      }
    }
    __syncthreads();
    if (view == 0 && tid == 0 && n_topview) n_topview[pr] = min(s_running, corr_cap);
  }
  __syncthreads();
  if (tid == 0) n[pr] = min(s_running, corr_cap);
}
__global__ __launch_bounds__(kThreads) void f2f_assemble_tracked_kernel(
    sosvo_rig rig, const float* __restrict__ m_top, const float* __restrict__ m_bot, const double* __restrict__ X,
    const int32_t* __restrict__ M, int frame_cap, const int32_t* __restrict__ ref_frame, const float* __restrict__ trk_top,
    const float* __restrict__ trk_bot, const uint8_t* __restrict__ st_top, const uint8_t* __restrict__ st_bot, int corr_cap,
    double* __restrict__ f, double* __restrict__ p, int32_t* __restrict__ cam, int32_t* __restrict__ corr_q,
    int32_t* __restrict__ corr_t, int32_t* __restrict__ n, int32_t* __restrict__ n_topview) {
  f2f_assemble_tracked_body<false>(rig, m_top, m_bot, X, M, frame_cap, ref_frame, trk_top, trk_bot, st_top, st_bot, corr_cap, f, p, cam, corr_q, corr_t,
                                   n, n_topview);
}
__global__ __launch_bounds__(kThreads) void f2f_assemble_tracked_cyclic_kernel(
    sosvo_rig rig, const float* __restrict__ m_top, const float* __restrict__ m_bot, const double* __restrict__ X,
    const int32_t* __restrict__ M, int frame_cap, const int32_t* __restrict__ ref_frame, const float* __restrict__ trk_top,
    const float* __restrict__ trk_bot, const uint8_t* __restrict__ st_top, const uint8_t* __restrict__ st_bot, int corr_cap,
    double* __restrict__ f, double* __restrict__ p, int32_t* __restrict__ cam, int32_t* __restrict__ corr_q,
    int32_t* __restrict__ corr_t, int32_t* __restrict__ n, int32_t* __restrict__ n_topview) {
  f2f_assemble_tracked_body<true>(rig, m_top, m_bot, X, M, frame_cap, ref_frame, trk_top, trk_bot, st_top, st_bot, corr_cap, f, p, cam, corr_q, corr_t,
                                   n, n_topview);
}

}  // namespace

// ---- host bodies shared by twin entry points: `fn` is the public function's name, for its messages

// what sosvo_stereo_assemble and sosvo_stereo_assemble_slots (table: its slot_of_frame) ask of their arguments
#define SOSVO_STEREO_ASSEMBLE_ARGS_OK(ctx, table)                                                                                  \
  SOSVO_REQUIRE(ctx, rig_host && kp_top && kp_bot && desc_top && desc_bot && n_top && n_bot && keys && order && (table),         \
                "null input pointer");                                                                                           \
  SOSVO_REQUIRE(ctx, m_top && m_bot && d_top && d_bot && X && b_top && b_bot && M, "null output pointer");                       \
  SOSVO_REQUIRE(ctx, nframes >= 0 && nframes <= (1 << 20) && nmask > 0 && cap > 0 && out_cap > 0, "sizes out of range");         \
  SOSVO_REQUIRE(ctx, cap <= (1 << SOSVO_KEY_SHIFT), "cap out of range")

// the cyclic gate's periods: the views' column counts, positive integers
static bool f2f_periods_ok(const sosvo_rig* rig) {
  const double a = rig->pano_top[0], b = rig->pano_bot[0];
  return a >= 1.0 && b >= 1.0 && a <= 16384.0 && b <= 16384.0 && a == floor(a) && b == floor(b);
}
#define SOSVO_F2F_PERIOD_MSG "the period (pano_top[0], pano_bot[0]) must be a positive integer up to 16384"

// sosvo_f2f_assemble and sosvo_f2f_assemble_cyclic
static int32_t f2f_assemble(sosvo_ctx* ctx, const char* fn, bool cyclic, const sosvo_rig* rig_host, const float* m_top,
                            const float* m_bot, const double* X, const double* b_top, const double* b_bot, const int32_t* M,
                            int32_t frame_cap, const int32_t* ref_frame, const int32_t* cur_frame, const uint32_t* keys_top,
                            const int32_t* order_top, const uint32_t* keys_bot, const int32_t* order_bot, int32_t npairs,
                            int32_t corr_cap, double* f, double* p, int32_t* cam, int32_t* corr_q, int32_t* corr_t, int32_t* n,
                            int32_t* n_topview) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE_FN(ctx, rig_host && m_top && m_bot && X && b_top && b_bot && M && ref_frame && cur_frame, "null input pointer");
  SOSVO_REQUIRE_FN(ctx, keys_top && order_top && keys_bot && order_bot && f && p && cam && corr_q && corr_t && n, "null pointer");
  SOSVO_REQUIRE_FN(ctx, npairs >= 0 && npairs <= (1 << 20) && frame_cap > 0 && corr_cap > 0, "sizes out of range");
  SOSVO_REQUIRE_FN(ctx, !cyclic || f2f_periods_ok(rig_host), SOSVO_F2F_PERIOD_MSG);
  if (npairs == 0) return SOSVO_OK;
  SOSVO_LAUNCH_AS(ctx, cyclic ? "f2f_assemble_cyclic_kernel" : "f2f_assemble_kernel", cyclic ? f2f_assemble_cyclic_kernel : f2f_assemble_kernel,
                  dim3(npairs), dim3(kThreads), 0, ctx->stream, *rig_host, m_top, m_bot, X, b_top, b_bot, M, frame_cap, ref_frame, cur_frame,
                  keys_top, order_top, keys_bot, order_bot, corr_cap, f, p, cam, corr_q, corr_t, n, n_topview);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

// sosvo_f2f_assemble_tracked and sosvo_f2f_assemble_tracked_cyclic
static int32_t f2f_assemble_tracked(sosvo_ctx* ctx, const char* fn, bool cyclic, const sosvo_rig* rig_host, const float* m_top,
                                    const float* m_bot, const double* X, const int32_t* M, int32_t frame_cap,
                                    const int32_t* ref_frame, const float* trk_top, const float* trk_bot, const uint8_t* st_top,
                                    const uint8_t* st_bot, int32_t npairs, int32_t corr_cap, double* f, double* p, int32_t* cam,
                                    int32_t* corr_q, int32_t* corr_t, int32_t* n, int32_t* n_topview) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE_FN(ctx, rig_host && m_top && m_bot && X && M && ref_frame && trk_top && trk_bot && st_top && st_bot,
                   "null input pointer");
  SOSVO_REQUIRE_FN(ctx, f && p && cam && corr_q && corr_t && n, "null output pointer");
  SOSVO_REQUIRE_FN(ctx, npairs >= 0 && npairs <= (1 << 20) && frame_cap > 0 && corr_cap > 0, "sizes out of range");
  SOSVO_REQUIRE_FN(ctx, !cyclic || f2f_periods_ok(rig_host), SOSVO_F2F_PERIOD_MSG);
  if (npairs == 0) return SOSVO_OK;
  SOSVO_LAUNCH_AS(ctx, cyclic ? "f2f_assemble_tracked_cyclic_kernel" : "f2f_assemble_tracked_kernel",
                  cyclic ? f2f_assemble_tracked_cyclic_kernel : f2f_assemble_tracked_kernel, dim3(npairs), dim3(kThreads), 0, ctx->stream,
                  *rig_host, m_top, m_bot, X, M, frame_cap, ref_frame, trk_top, trk_bot, st_top, st_bot, corr_cap, f, p, cam, corr_q, corr_t,
                  n, n_topview);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

extern "C" {

int32_t sosvo_pano_to_bearing(sosvo_ctx* ctx, const double* uv, int32_t n, double cols, double rows,
                              double pixel_size, double cyl_height_max, double* az, double* el, double* bearing) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, uv && n >= 0, "bad arguments");
  if (n == 0) return SOSVO_OK;
  SOSVO_LAUNCH(ctx,pano_to_bearing_kernel, dim3(cdiv(n, kThreads)), dim3(kThreads), 0, ctx->stream, uv, n, cols, rows,
                     pixel_size, cyl_height_max, az, el, bearing);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

int32_t sosvo_triangulate_midpoint(sosvo_ctx* ctx, const double* az_top, const double* el_top, const double* az_bot,
                                   const double* el_bot, int32_t n, const double* F_top_host,
                                   const double* F_bot_host, double* X) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, az_top && el_top && az_bot && el_bot && F_top_host && F_bot_host && X && n >= 0, "bad arguments");
  if (n == 0) return SOSVO_OK;
  F3x2 foci;
  for (int k = 0; k < 3; ++k) {
    foci.F1[k] = F_top_host[k];
    foci.F2[k] = F_bot_host[k];
  }
  SOSVO_LAUNCH(ctx,triangulate_kernel, dim3(cdiv(n, kThreads)), dim3(kThreads), 0, ctx->stream, az_top, el_top, az_bot,
                     el_bot, n, foci, X);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

int32_t sosvo_triangulate2(sosvo_ctx* ctx, const double* b1, const double* b2, int32_t n, const double* t12_host,
                           const double* R12_host, double* X) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, b1 && b2 && t12_host && R12_host && X && n >= 0, "bad arguments");
  if (n == 0) return SOSVO_OK;
  Rt12 rt;
  for (int k = 0; k < 3; ++k) rt.t[k] = t12_host[k];
  for (int k = 0; k < 9; ++k) rt.R[k] = R12_host[k];
  SOSVO_LAUNCH(ctx, triangulate2_kernel, dim3(cdiv(n, kThreads)), dim3(kThreads), 0, ctx->stream, b1, b2, n, rt, X);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

int32_t sosvo_range_filter(sosvo_ctx* ctx, const double* X, int32_t n, double min_range, double max_range,
                           uint8_t* ok) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, X && ok && n >= 0, "bad arguments");
  if (n == 0) return SOSVO_OK;
  SOSVO_LAUNCH(ctx,range_filter_kernel, dim3(cdiv(n, kThreads)), dim3(kThreads), 0, ctx->stream, X, n, min_range,
                     max_range, ok);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

int32_t sosvo_rgbd_backproject(sosvo_ctx* ctx, const float* depth, int32_t rows, int32_t cols, const int32_t* u,
                               const int32_t* v, int32_t n, double fx, double fy, double cx, double cy,
                               double focal_length_m, int32_t depth_is_Z, double* xyz, double* bearing) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, depth && u && v && xyz && bearing && n >= 0 && rows > 0 && cols > 0, "bad arguments");
  if (n == 0) return SOSVO_OK;
  Intr k{fx, fy, cx, cy, focal_length_m};
  SOSVO_LAUNCH(ctx,rgbd_backproject_kernel, dim3(cdiv(n, kThreads)), dim3(kThreads), 0, ctx->stream, depth, rows, cols,
                     u, v, n, k, depth_is_Z, xyz, bearing);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

int32_t sosvo_stereo_assemble(sosvo_ctx* ctx, const sosvo_rig* rig_host, const float* kp_top, const float* kp_bot,
                              const uint8_t* desc_top, const uint8_t* desc_bot, const int32_t* n_top,
                              const int32_t* n_bot, const uint32_t* keys, const int32_t* order, int32_t nframes,
                              int32_t nmask, int32_t cap, int32_t out_cap, float* m_top, float* m_bot, uint8_t* d_top,
                              uint8_t* d_bot, double* X, double* b_top, double* b_bot, int32_t* M, int32_t* n_cand) {
  SOSVO_ENTER(ctx);
  SOSVO_STEREO_ASSEMBLE_ARGS_OK(ctx, true);
  if (nframes == 0) return SOSVO_OK;
  SOSVO_LAUNCH(ctx,stereo_assemble_kernel, dim3(nframes), dim3(kThreads), 0, ctx->stream, *rig_host, kp_top, kp_bot,
                     reinterpret_cast<const uint4*>(desc_top), reinterpret_cast<const uint4*>(desc_bot), n_top, n_bot,
                     keys, order, nmask, cap, out_cap, m_top, m_bot, reinterpret_cast<uint4*>(d_top),
                     reinterpret_cast<uint4*>(d_bot), X, b_top, b_bot, M, n_cand);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

// (internal, common.h) sosvo_stereo_assemble with the record of frame i written at record slot_of_frame[i] of the outputs
// (HOST table, checked by the caller: distinct records inside the outputs)
int32_t sosvo_stereo_assemble_slots(sosvo_ctx* ctx, const sosvo_rig* rig_host, const float* kp_top, const float* kp_bot,
                                    const uint8_t* desc_top, const uint8_t* desc_bot, const int32_t* n_top,
                                    const int32_t* n_bot, const uint32_t* keys, const int32_t* order, int32_t nframes,
                                    const int32_t* slot_of_frame, int32_t nmask, int32_t cap, int32_t out_cap, float* m_top,
                                    float* m_bot, uint8_t* d_top, uint8_t* d_bot, double* X, double* b_top, double* b_bot,
                                    int32_t* M, int32_t* n_cand) {
  SOSVO_STEREO_ASSEMBLE_ARGS_OK(ctx, slot_of_frame);
  for (int f0 = 0; f0 < nframes; f0 += kSosvoSlotArgFrames) {
    const int nf = nframes - f0 < kSosvoSlotArgFrames ? nframes - f0 : kSosvoSlotArgFrames;
    sosvo_slot_table tab;
    for (int i = 0; i < kSosvoSlotArgFrames; ++i) tab.slot[i] = i < nf ? slot_of_frame[f0 + i] : 0;
    SOSVO_LAUNCH(ctx, stereo_assemble_slots_kernel, dim3(nf), dim3(kThreads), 0, ctx->stream, *rig_host, tab, f0, kp_top, kp_bot,
                 reinterpret_cast<const uint4*>(desc_top), reinterpret_cast<const uint4*>(desc_bot), n_top, n_bot, keys, order,
                 nmask, cap, out_cap, m_top, m_bot, reinterpret_cast<uint4*>(d_top), reinterpret_cast<uint4*>(d_bot), X, b_top,
                 b_bot, M, n_cand);
    SOSVO_LAUNCH_CHECK(ctx);
  }
  return SOSVO_OK;
}

int32_t sosvo_f2f_assemble_cyclic(sosvo_ctx* ctx, const sosvo_rig* rig_host, const float* m_top, const float* m_bot,
                                  const double* X, const double* b_top, const double* b_bot, const int32_t* M,
                                  int32_t frame_cap, const int32_t* ref_frame, const int32_t* cur_frame,
                                  const uint32_t* keys_top, const int32_t* order_top, const uint32_t* keys_bot,
                                  const int32_t* order_bot, int32_t npairs, int32_t corr_cap, double* f, double* p,
                                  int32_t* cam, int32_t* corr_q, int32_t* corr_t, int32_t* n, int32_t* n_topview) {
  return f2f_assemble(ctx, __func__, true, rig_host, m_top, m_bot, X, b_top, b_bot, M, frame_cap, ref_frame, cur_frame, keys_top,
                      order_top, keys_bot, order_bot, npairs, corr_cap, f, p, cam, corr_q, corr_t, n, n_topview);
}

int32_t sosvo_f2f_assemble(sosvo_ctx* ctx, const sosvo_rig* rig_host, const float* m_top, const float* m_bot,
                           const double* X, const double* b_top, const double* b_bot, const int32_t* M,
                           int32_t frame_cap, const int32_t* ref_frame, const int32_t* cur_frame,
                           const uint32_t* keys_top, const int32_t* order_top, const uint32_t* keys_bot,
                           const int32_t* order_bot, int32_t npairs, int32_t corr_cap, double* f, double* p,
                           int32_t* cam, int32_t* corr_q, int32_t* corr_t, int32_t* n, int32_t* n_topview) {
  return f2f_assemble(ctx, __func__, false, rig_host, m_top, m_bot, X, b_top, b_bot, M, frame_cap, ref_frame, cur_frame, keys_top,
                      order_top, keys_bot, order_bot, npairs, corr_cap, f, p, cam, corr_q, corr_t, n, n_topview);
}

int32_t sosvo_f2f_assemble_tracked(sosvo_ctx* ctx, const sosvo_rig* rig_host, const float* m_top, const float* m_bot,
                                   const double* X, const int32_t* M, int32_t frame_cap, const int32_t* ref_frame,
                                   const float* trk_top, const float* trk_bot, const uint8_t* st_top, const uint8_t* st_bot,
                                   int32_t npairs, int32_t corr_cap, double* f, double* p, int32_t* cam, int32_t* corr_q,
                                   int32_t* corr_t, int32_t* n, int32_t* n_topview) {
  return f2f_assemble_tracked(ctx, __func__, false, rig_host, m_top, m_bot, X, M, frame_cap, ref_frame, trk_top, trk_bot, st_top,
                              st_bot, npairs, corr_cap, f, p, cam, corr_q, corr_t, n, n_topview);
}

int32_t sosvo_f2f_assemble_tracked_cyclic(sosvo_ctx* ctx, const sosvo_rig* rig_host, const float* m_top, const float* m_bot,
                                          const double* X, const int32_t* M, int32_t frame_cap, const int32_t* ref_frame,
                                          const float* trk_top, const float* trk_bot, const uint8_t* st_top,
                                          const uint8_t* st_bot, int32_t npairs, int32_t corr_cap, double* f, double* p,
                                          int32_t* cam, int32_t* corr_q, int32_t* corr_t, int32_t* n, int32_t* n_topview) {
  return f2f_assemble_tracked(ctx, __func__, true, rig_host, m_top, m_bot, X, M, frame_cap, ref_frame, trk_top, trk_bot, st_top,
                              st_bot, npairs, corr_cap, f, p, cam, corr_q, corr_t, n, n_topview);
}

}  // extern "C"
