// sosvo_gray_pyramid, sosvo_track_lk -- cv2.calcOpticalFlowPyrLK restated in exact integers: the points
// of one gray image are tracked into another, coarse to fine over a pyramid of up to four levels.  sosvo_refine_stereo_lk
// (section 29) is the same tracker at one level between the two views of a frame, behind a gather and before an acceptance.
//
// Per point and level: the template T is (2 half + 3)^2 integer bilinear samples on the 1/32-px grid (at most 255 * 1024),
// its Scharr gradients are integers below 2^22, the normal equations A, B, C and the right-hand sides b1, b2 of every
// iteration are int64 sums (below 2^53 / 2^49).  Exact integers: the sums do not depend on which lane adds what, and the CPU
// reference (tests/reflk.py) gets the same bits.  Only the minimum eigenvalue, the 2 x 2 solve and the position arithmetic are
// floating point -- FP64, every sum converted once, no contraction, a correctly rounded square root -- and every lane of a
// keypoint's group evaluates them on the same values.
//
// MAPPING.  A workgroup is one wave.  A keypoint owns a GROUP of GS lanes: 16 lanes for half 2 .. 5 (25 .. 121 window elements,
// four keypoints per wave), the whole wave for half 6 .. 10 (169 .. 441 elements).  Lane r of a group owns the window elements
// r, r + GS, ... for all iterations.  The groups of a wave run in lockstep: loops have wave-uniform bounds and a group that is
// done is predicated off, so the group reductions (xor shuffles below GS) always see every lane.
//
// LDS per group: the template with its one-pixel halo (pitch 2 half + 3, read once per level for the gradients) and three DENSE
// planes of (2 half + 1)^2 int32 -- the template's window, gx, gy -- that every iteration reads at element index e: lane r of
// a group reads word base + r + k GS, consecutive lanes consecutive banks.  A group's block is 16 words more than a multiple
// of 32, so the two 16-lane groups that share a 32-lane half of a ds_read_b32 sit on opposite halves of the 32 banks.
#include <math.h>

#include "common.h"

namespace {

constexpr int kLkMaxHalf = 10;
constexpr int kLkMaxLevels = 4;
constexpr int kPyrTileX = 32, kPyrTileY = 8;  // output pixels of one pyramid workgroup

// ---- the levels of a pyramid set ---------------------------------------------------------------------------------------------
struct LkLevels {
  const uint8_t* base[kLkMaxLevels];  // level l as [nimg, rows[l], cols[l]]
  int32_t rows[kLkMaxLevels], cols[kLkMaxLevels];
};

// bytes of the levels 1 .. levels - 1 of nimg images (what sosvo_gray_pyramid writes), and their table
int64_t lk_levels(const uint8_t* gray, const uint8_t* pyr, int nimg, int rows, int cols, int levels, LkLevels* t) {
  int64_t off = 0;
  for (int l = 0; l < kLkMaxLevels; ++l) {
    const bool above = l >= 1 && l < levels;
    if (t) {
      t->base[l] = l == 0 ? gray : (above ? pyr + off : nullptr);
      t->rows[l] = rows;
      t->cols[l] = cols;
    }
    if (above) off += (int64_t)nimg * rows * cols;
    rows = (rows + 1) / 2;
    cols = (cols + 1) / 2;
  }
  return off;
}

// The rows [r0, r1) of level `level` that belong to the view's row range (row_range = nullptr: all rows).  Level 0: the range
// cut to the image and to at least one row; level l + 1: [(r0 + 1) / 2, max((r1 + 1) / 2, that + 1)), cut to the level.
__device__ __forceinline__ void lk_level_rows(const int32_t* __restrict__ row_range, int view, int rows0, int level, int* r0_out,
                                              int* r1_out) {
  int r0 = 0, r1 = rows0;
  if (row_range) {
    r0 = clampi(row_range[2 * view], 0, rows0 - 1);
    r1 = clampi(row_range[2 * view + 1], r0 + 1, rows0);
  }
  int rows = rows0;
  for (int l = 0; l < level; ++l) {
    rows = (rows + 1) / 2;
    r0 = min((r0 + 1) / 2, rows - 1);  // (a range that is the last row of an even level: cut to the level, as at level 0)
    r1 = min(max((r1 + 1) / 2, r0 + 1), rows);
  }
  *r0_out = r0;
  *r1_out = r1;
}

// ---- one pyramid level: (sum k_i k_j in[clamp(2 y + i)][clamp(2 x + j)] + 128) >> 8, k = (1, 4, 6, 4, 1) --------------------
// (the tile blockIdx.x, blockIdx.y of image `image`, which belongs to view `view` of the row range)
// CYC (sosvo_gray_pyramid_cyclic): the column index is (2 x + j) mod cols_in, cols_in even.  An output
// column reads the columns -2 .. cols_in of the level below: one conditional add per side wraps them; the clamp behind it only
// keeps the loads of a tile's lanes beyond the level (never used) inside the row.
template <bool CYC = false>
__device__ __forceinline__ void lk_pyr_down_tile(const uint8_t* __restrict__ in, int rows_in, int cols_in, uint8_t* __restrict__ out,
                                                 int rows_out, int cols_out, const int32_t* __restrict__ row_range, int image, int view,
                                                 int rows0, int level_in) {
  constexpr int TW = 2 * kPyrTileX + 3, TH = 2 * kPyrTileY + 3;
  __shared__ uint8_t s_in[TH][TW + 1];
  int ri0, ri1, ro0, ro1;
  lk_level_rows(row_range, view, rows0, level_in, &ri0, &ri1);
  lk_level_rows(row_range, view, rows0, level_in + 1, &ro0, &ro1);
  ri1 = min(ri1, rows_in);  // (the formula never exceeds the level; belt and braces for the reads)
  ro1 = min(ro1, rows_out);
  const int x0 = blockIdx.x * kPyrTileX, y0 = blockIdx.y * kPyrTileY;
  if (y0 >= ro1 || y0 + kPyrTileY <= ro0) return;  // (uniform) no row of this tile is in the range
  const uint8_t* src = in + (size_t)image * rows_in * cols_in;
  const int tid = threadIdx.y * kPyrTileX + threadIdx.x;
  for (int s = tid; s < TH * TW; s += kPyrTileX * kPyrTileY) {
    const int i = s / TW, j = s - i * TW;
    const int y = clampi(2 * y0 - 2 + i, ri0, ri1 - 1);
    int x = 2 * x0 - 2 + j;
    if constexpr (CYC) {
      x += x < 0 ? cols_in : 0;
      x -= x >= cols_in ? cols_in : 0;
    }
    x = clampi(x, 0, cols_in - 1);
    s_in[i][j] = src[(size_t)y * cols_in + x];
  }
  __syncthreads();
  const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
  if (x >= cols_out || y < ro0 || y >= ro1) return;
  const int k[5] = {1, 4, 6, 4, 1};
  int sum = 128;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    int row = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) row += k[j] * s_in[2 * threadIdx.y + i][2 * threadIdx.x + j];
    sum += k[i] * row;
  }
  out[((size_t)image * rows_out + y) * cols_out + x] = (uint8_t)(sum >> 8);
}

__global__ __launch_bounds__(kPyrTileX* kPyrTileY) void lk_pyr_down_kernel(const uint8_t* __restrict__ in, int rows_in, int cols_in,
                                                                          uint8_t* __restrict__ out, int rows_out, int cols_out,
                                                                          const int32_t* __restrict__ row_range, int imgs_per_range,
                                                                          int rows0, int level_in) {
  const int image = blockIdx.z;
  lk_pyr_down_tile(in, rows_in, cols_in, out, rows_out, cols_out, row_range, image, image / imgs_per_range, rows0, level_in);
}

__global__ __launch_bounds__(kPyrTileX* kPyrTileY) void lk_pyr_down_cyclic_kernel(const uint8_t* __restrict__ in, int rows_in, int cols_in,
                                                                                 uint8_t* __restrict__ out, int rows_out, int cols_out,
                                                                                 const int32_t* __restrict__ row_range,
                                                                                 int imgs_per_range, int rows0, int level_in) {
  const int image = blockIdx.z;
  lk_pyr_down_tile<true>(in, rows_in, cols_in, out, rows_out, cols_out, row_range, image, image / imgs_per_range, rows0, level_in);
}

// ---- the images of a frame store (SOSVO_FLAG_LK_F2F) ----------------------------------------------------
// A store of `slots` frames keeps level l as [2 * slots, rows_l, cols_l], view-major: image v * slots + s is view v of slot s,
// so the kernels above and the tracker see one pyramid set of nimg = 2 * slots images under the views' row range.  A front
// end over nf frames has its gray rows as [2, nf_all, rows, cols]; frame f0 + i of it goes to slot tab.slot[i].
//
// Level 0: the rows of the view's range, copied (workgroup (c, i, v) takes every gridDim.x-th 4 KB block of the span).
__global__ __launch_bounds__(256) void lk_store_level0_kernel(const uint8_t* __restrict__ gray, int nf_all, int f0, sosvo_slot_table tab,
                                                              int slots, int rows, int cols, const int32_t* __restrict__ row_range,
                                                              uint8_t* __restrict__ level0) {
  const int i = blockIdx.y, v = blockIdx.z;
  int r0, r1;
  lk_level_rows(row_range, v, rows, 0, &r0, &r1);
  const size_t npx = (size_t)rows * cols, first = (size_t)r0 * cols, bytes = (size_t)(r1 - r0) * cols;
  sosvo_copy_bytes(level0 + ((size_t)v * slots + tab.slot[i]) * npx + first, gray + ((size_t)v * nf_all + f0 + i) * npx + first, bytes,
                   blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}
// ... from a front end that ran on padded panoramas (SOSVO_FLAG_SEAM_FREE): gray rows are cols + 2 pad bytes
// long and the store takes their interior, the columns [pad, pad + cols).
__global__ __launch_bounds__(256) void lk_store_level0_padded_kernel(const uint8_t* __restrict__ gray, int nf_all, int f0,
                                                                     sosvo_slot_table tab, int slots, int rows, int cols, int pad,
                                                                     const int32_t* __restrict__ row_range, uint8_t* __restrict__ level0) {
  const int i = blockIdx.y, v = blockIdx.z;
  int r0, r1;
  lk_level_rows(row_range, v, rows, 0, &r0, &r1);
  const size_t pitch = (size_t)cols + 2 * pad;
  sosvo_copy_rows(level0 + (((size_t)v * slots + tab.slot[i]) * rows + r0) * cols, (size_t)cols,
                  gray + (((size_t)v * nf_all + f0 + i) * rows + r0) * pitch + pad, pitch, cols, r1 - r0,
                  blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}
// Level l + 1 from level l, both in the store: blockIdx.z = v * nf + i is view v of slot tab.slot[i].
__global__ __launch_bounds__(kPyrTileX* kPyrTileY) void lk_pyr_down_slots_kernel(const uint8_t* __restrict__ in, int rows_in, int cols_in,
                                                                                uint8_t* __restrict__ out, int rows_out, int cols_out,
                                                                                const int32_t* __restrict__ row_range, int nf,
                                                                                sosvo_slot_table tab, int slots, int rows0, int level_in) {
  const int v = blockIdx.z / nf, i = blockIdx.z - v * nf;
  lk_pyr_down_tile(in, rows_in, cols_in, out, rows_out, cols_out, row_range, v * slots + tab.slot[i], v, rows0, level_in);
}
__global__ __launch_bounds__(kPyrTileX* kPyrTileY) void lk_pyr_down_slots_cyclic_kernel(const uint8_t* __restrict__ in, int rows_in,
                                                                                       int cols_in, uint8_t* __restrict__ out,
                                                                                       int rows_out, int cols_out,
                                                                                       const int32_t* __restrict__ row_range, int nf,
                                                                                       sosvo_slot_table tab, int slots, int rows0,
                                                                                       int level_in) {
  const int v = blockIdx.z / nf, i = blockIdx.z - v * nf;
  lk_pyr_down_tile<true>(in, rows_in, cols_in, out, rows_out, cols_out, row_range, v * slots + tab.slot[i], v, rows0, level_in);
}

// ---- the tracker -------------------------------------------------------------------------------------------------------------
template <int GS>
__device__ __forceinline__ long long group_sum(long long v) {
#pragma unroll
  for (int s = GS / 2; s > 0; s >>= 1) v += __shfl_xor(v, s);
  return v;
}

// the integer bilinear sample of a level at pixel (x, y) + (fx, fy) / 32, coordinates clamped to the columns and to the rows
// [r0, r1) of the level
// CYC: the two column taps are x mod cols and (x + 1) mod cols.  x lies within half + 2 columns of a base in [0, cols) and the
// top level holds at least 2 half + 3 columns (the entry point checks it), so one conditional add per side is the modulo.
template <bool CYC = false>
__device__ __forceinline__ int lk_sample(const uint8_t* __restrict__ img, int cols, int r0, int r1, int x, int y, int fx, int fy) {
  int xa, xb;
  if constexpr (CYC) {
    xa = x + (x < 0 ? cols : 0);
    xa -= xa >= cols ? cols : 0;
    xb = xa + 1;
    xb -= xb >= cols ? cols : 0;
  } else {
    xa = clampi(x, 0, cols - 1);
    xb = clampi(x + 1, 0, cols - 1);
  }
  const int ya = clampi(y, r0, r1 - 1), yb = clampi(y + 1, r0, r1 - 1);
  const int p00 = img[(size_t)ya * cols + xa], p01 = img[(size_t)ya * cols + xb];
  const int p10 = img[(size_t)yb * cols + xa], p11 = img[(size_t)yb * cols + xb];
  return (32 - fy) * ((32 - fx) * p00 + fx * p01) + fy * ((32 - fx) * p10 + fx * p11);
}

// A position on the 1/32-px grid of a level: tq = floor(32 c + 0.5) per axis; inside = the rounded position lies in
// [0, cols - 1] x [r0, r1 - 1] (false for NaN); then base and fraction are small integers.
struct LkGrid {
  double tqx, tqy;
  int bx, by, fx, fy;
  bool inside;
};
// CYC: tqx is reduced to [0, 32 cols) -- tq - P floor(tq / P), P = 32 cols: exact, tq is an integer below 2^40 and P one of at
// most 2^19, so the quotient's rounding (below 2^-17) never reaches the next integer from a fraction of at least 1 / P -- and
// "inside" is a matter of the rows; a non-finite value or |32 x + 0.5| >= 2^40 is outside, as it is without CYC.
template <bool CYC = false>
__device__ __forceinline__ LkGrid lk_grid(double cx, double cy, int cols, int r0, int r1) {
  LkGrid g;
  g.tqx = floor(32.0 * cx + 0.5);
  g.tqy = floor(32.0 * cy + 0.5);
  if constexpr (CYC) {
    const double period = 32.0 * (double)cols;
    const bool okx = fabs(32.0 * cx + 0.5) < 1099511627776.0;  // (false for NaN)
    // (a guess one step away from a reduced position lies within a period of [0, P): one conditional add per side is the
    // reduction; the division serves the rest -- a start or a guess from anywhere, a step of a period or more.  Same value.)
    double t = g.tqx;
    if (t >= -period && t < 2.0 * period) {
      t += t < 0.0 ? period : 0.0;
      t -= t >= period ? period : 0.0;
    } else {
      t = t - period * floor(t / period);
    }
    g.tqx = okx ? t : 0.0;
    g.inside = okx && g.tqy >= 32.0 * (double)r0 && g.tqy <= 32.0 * (double)(r1 - 1);
  } else {
    g.inside = g.tqx >= 0.0 && g.tqx <= 32.0 * (double)(cols - 1) && g.tqy >= 32.0 * (double)r0 && g.tqy <= 32.0 * (double)(r1 - 1);
  }
  const int qx = g.inside ? (int)g.tqx : 0, qy = g.inside ? (int)g.tqy : 0;
  g.bx = qx >> 5;
  g.fx = qx & 31;
  g.by = qy >> 5;
  g.fy = qy & 31;
  return g;
}

struct LkArgs {
  LkLevels lv;
  int nimg, levels, cap, half, max_iter, initial_flow;
  double eps2, min_eig, fb_max2;  // fb_max2 < 0: the forward pass
};

// Words of LDS of one group: the halo'd template, three dense planes, rounded up to 16 more than a multiple of 32.
__host__ __device__ constexpr int lk_group_words(int half) {
  const int side3 = 2 * half + 3, side1 = 2 * half + 1;
  return ((side3 * side3 + 3 * side1 * side1 + 31) / 32) * 32 + 16;
}
constexpr int kLkLdsWords16 = 4 * lk_group_words(5), kLkLdsWords64 = lk_group_words(kLkMaxHalf);

// The FORWARD pass (a.fb_max2 < 0) tracks start = prev_pts (guess: next_pts with the initial-flow flag) from image prev_img[p] to
// image next_img[p] and writes next_pts, status, err.  The BACKWARD pass (a.fb_max2 >= 0) is launched with the images swapped
// and start = the forward results: points whose status is 1 are tracked back, `out` = back receives the position (the start
// for the others), and the status is cleared where the point is lost or |back - ref|^2 > fb_max^2 (ref = the forward start).
// store_pt (nullptr: the points of problem p are the rows p * cap ...): the forward start points -- `start` of the forward pass,
// `ref` of the backward pass -- are read where they lie, problem p's from point store_pt[p] on (a frame store's m_top / m_bot).
//
// CYC (SOSVO_LK_CYCLIC_COLUMNS): the columns are one period.  Rounded x positions and column taps wrap
// (lk_grid, lk_sample), a position is never "outside" by its x, the x written is g.x - W floor(g.x / W) (W = level 0's columns;
// a float that rounds up to W is written as 0), and the backward pass measures x the short way round.  Everything else is
// the text below, shared.
template <int GS, bool CYC = false>
__global__ __launch_bounds__(64) void lk_track_kernel(LkArgs a, const int32_t* __restrict__ row_range, const int32_t* __restrict__ from_img,
                                                      const int32_t* __restrict__ to_img, const float* __restrict__ start,
                                                      const int32_t* __restrict__ n, float* __restrict__ out,
                                                      uint8_t* __restrict__ status, float* __restrict__ err,
                                                      const float* __restrict__ ref, const int64_t* __restrict__ store_pt) {
  constexpr int KPW = 64 / GS;  // keypoints per wave
  __shared__ int32_t s_lds[GS == 64 ? kLkLdsWords64 : kLkLdsWords16];
  const int lane = threadIdx.x, grp = lane / GS, r = lane - grp * GS;
  const int p = blockIdx.x;
  const int img_a = from_img[p], img_b = to_img[p];
  if (img_a < 0 || img_a >= a.nimg || img_b < 0 || img_b >= a.nimg) return;  // (uniform) no such image: the problem is ignored
  const int count = min(__builtin_amdgcn_readfirstlane(n[p]), a.cap);
  const int half = a.half, side3 = 2 * half + 3, side1 = 2 * half + 1, N = side1 * side1;
  const bool backward = a.fb_max2 >= 0.0;
  const int imgs_per_range = a.nimg > 1 ? a.nimg / 2 : 1;
  const int view_a = row_range ? img_a / imgs_per_range : 0, view_b = row_range ? img_b / imgs_per_range : 0;
  int32_t* s_T = s_lds + grp * lk_group_words(GS == 64 ? kLkMaxHalf : 5);
  int32_t* s_Tc = s_T + side3 * side3;
  int32_t* s_gx = s_Tc + N;
  int32_t* s_gy = s_gx + N;
  const double den = (double)N * 2147483648.0;  // 2 N 2^30

  for (int k0 = blockIdx.y * KPW; k0 < count; k0 += gridDim.y * KPW) {  // (uniform)
    const int k = k0 + grp;
    const size_t row = (size_t)p * a.cap + min(k, count - 1);
    const size_t srow = store_pt && !backward ? (size_t)store_pt[p] + min(k, count - 1) : row;
    const float sx = start[2 * srow], sy = start[2 * srow + 1];
    float gx0 = sx, gy0 = sy;
    if (a.initial_flow) {
      gx0 = out[2 * row];
      gy0 = out[2 * row + 1];
    }
    // `live`: this group tracks a point.  `lost` is final once set.
    bool live = k < count && isfinite(sx) && isfinite(sy) && isfinite(gx0) && isfinite(gy0);
    if (backward) live = live && status[row] != 0;
    const bool skipped = k < count && !live;  // not tracked: the result is the start
    bool lost = false;
    const double px = (double)sx, py = (double)sy;
    const double top = 1.0 / (double)(1 << (a.levels - 1));
    double cx = (double)gx0 * top, cy = (double)gy0 * top;  // the guess at the current level
    long long err_sum = 0;

    for (int l = a.levels - 1; l >= 0; --l) {  // (uniform)
      const int cols = a.lv.cols[l], rows = a.lv.rows[l];
      int ra0, ra1, rb0, rb1;
      lk_level_rows(row_range, view_a, a.lv.rows[0], l, &ra0, &ra1);
      lk_level_rows(row_range, view_b, a.lv.rows[0], l, &rb0, &rb1);
      ra1 = min(ra1, rows);
      rb1 = min(rb1, rows);
      const uint8_t* ia = a.lv.base[l] + (size_t)img_a * rows * cols;
      const uint8_t* ib = a.lv.base[l] + (size_t)img_b * rows * cols;
      const double scale = 1.0 / (double)(1 << l);
      const LkGrid t = lk_grid<CYC>(px * scale, py * scale, cols, ra0, ra1);
      bool run = live && !lost && t.inside;  // this group iterates at this level
      if (live && !lost && !t.inside && l == 0) lost = true;
      // ---- the template and its gradients
      if (run) {
        for (int s = r; s < side3 * side3; s += GS) {
          const int i = s / side3, j = s - i * side3;
          s_T[s] = lk_sample<CYC>(ia, cols, ra0, ra1, t.bx + j - half - 1, t.by + i - half - 1, t.fx, t.fy);
        }
      }
      __syncthreads();
      long long sa = 0, sb = 0, sc = 0;
      if (run) {
        for (int e = r; e < N; e += GS) {
          const int i = e / side1, j = e - i * side1;
          const int32_t* q = s_T + i * side3 + j;  // q[0] = T[i][j] of the halo'd template, the window element is q[side3 + 1]
          const int t00 = q[0], t01 = q[1], t02 = q[2];
          const int t10 = q[side3], t12 = q[side3 + 2];
          const int t20 = q[2 * side3], t21 = q[2 * side3 + 1], t22 = q[2 * side3 + 2];
          const int gx = 3 * (t02 - t00) + 10 * (t12 - t10) + 3 * (t22 - t20);
          const int gy = 3 * (t20 - t00) + 10 * (t21 - t01) + 3 * (t22 - t02);
          s_Tc[e] = q[side3 + 1];
          s_gx[e] = gx;
          s_gy[e] = gy;
          sa += (long long)gx * gx;
          sb += (long long)gx * gy;
          sc += (long long)gy * gy;
        }
      }
      const double A = (double)group_sum<GS>(sa), B = (double)group_sum<GS>(sb), C = (double)group_sum<GS>(sc);
      const double det = A * C - B * B;
      const double diff = A - C;
      const double eig = (A + C - __dsqrt_rn(diff * diff + 4.0 * B * B)) / den;
      if (run && (det == 0.0 || eig < a.min_eig)) {  // no texture: the point is lost at level 0, the level is skipped above it
        run = false;
        if (l == 0) lost = true;
      }
      // ---- the iteration
      double pdx = 0.0, pdy = 0.0;
      bool iterating = run;
      for (int it = 0; it < a.max_iter; ++it) {  // (uniform bound; left when no group of the wave iterates)
        if (!__any(iterating)) break;
        const LkGrid g = lk_grid<CYC>(cx, cy, cols, rb0, rb1);
        if (iterating && !g.inside) {  // left the image: lost at level 0, the end of this level above it
          iterating = false;
          if (l == 0) lost = true;
        }
        long long s1 = 0, s2 = 0;
        if (iterating) {
          for (int e = r; e < N; e += GS) {
            const int i = e / side1, j = e - i * side1;
            const long long d = lk_sample<CYC>(ib, cols, rb0, rb1, g.bx + j - half, g.by + i - half, g.fx, g.fy) - s_Tc[e];
            s1 += d * s_gx[e];
            s2 += d * s_gy[e];
          }
        }
        const double b1 = (double)group_sum<GS>(s1), b2 = (double)group_sum<GS>(s2);
        if (iterating) {
          const double dx = -32.0 * (C * b1 - B * b2) / det, dy = -32.0 * (A * b2 - B * b1) / det;
          cx = g.tqx * 0.03125 + dx;
          cy = g.tqy * 0.03125 + dy;
          if (dx * dx + dy * dy <= a.eps2) {
            iterating = false;
          } else if (it > 0 && fabs(dx + pdx) < 0.01 && fabs(dy + pdy) < 0.01) {  // oscillation: half the step back
            cx -= dx * 0.5;
            cy -= dy * 0.5;
            iterating = false;
          } else if (floor(32.0 * cx + 0.5) == g.tqx && floor(32.0 * cy + 0.5) == g.tqy) {
            // The new guess rounds to the position this step was taken from: the next iteration would sample the same J and
            // take the same step, and so would every one after it.  (The step is measured from the ROUNDED guess, so at the
            // fixed point it is the solution's distance to the grid, up to 1/64 px: the eps stop fires only within eps of a grid
            // point.)  What those iterations would do is known now: the oscillation rule at the next one, if there is one,
            // sees 2 dx and 2 dy; otherwise nothing changes up to max_iter.  Same bits, without running them.
            if (it + 1 < a.max_iter && fabs(dx + dx) < 0.01 && fabs(dy + dy) < 0.01) {
              cx -= dx * 0.5;
              cy -= dy * 0.5;
            }
            iterating = false;
          }
          pdx = dx;
          pdy = dy;
        }
      }
      if (l > 0) {
        cx *= 2.0;
        cy *= 2.0;
      } else {
        // ---- the residual at the final rounded position
        const LkGrid g = lk_grid<CYC>(cx, cy, cols, rb0, rb1);
        const bool ok = live && !lost && g.inside;
        if (live && !lost && !g.inside) lost = true;
        long long s = 0;
        if (ok) {
          for (int e = r; e < N; e += GS) {
            const int i = e / side1, j = e - i * side1;
            const int d = lk_sample<CYC>(ib, cols, rb0, rb1, g.bx + j - half, g.by + i - half, g.fx, g.fy) - s_Tc[e];
            s += d < 0 ? -d : d;
          }
        }
        err_sum = group_sum<GS>(s);
      }
      __syncthreads();  // (the next level / keypoint writes the template)
    }

    if (r == 0 && k < count) {
      const size_t o = (size_t)p * a.cap + k;
      if (skipped) {
        out[2 * o] = sx;
        out[2 * o + 1] = sy;
        if (!backward) {
          status[o] = 0;
          err[o] = 0.0f;
        }
      } else {
        float ox = (float)cx;
        const float oy = (float)cy;
        if constexpr (CYC) {
          const double W = (double)a.lv.cols[0];
          ox = (float)(cx - W * floor(cx / W));
          if (ox == (float)W) ox = 0.0f;
        }
        out[2 * o] = ox;
        out[2 * o + 1] = oy;
        if (!backward) {
          status[o] = lost ? 0 : 1;
          err[o] = lost ? 0.0f : (float)((double)err_sum / (1024.0 * (double)N));
        } else {
          const size_t ro = store_pt ? (size_t)store_pt[p] + k : o;
          double ddx = (double)ox - (double)ref[2 * ro];
          const double ddy = (double)oy - (double)ref[2 * ro + 1];
          if constexpr (CYC) ddx = fmin(fabs(ddx), (double)a.lv.cols[0] - fabs(ddx));
          if (lost || !(ddx * ddx + ddy * ddy <= a.fb_max2)) status[o] = 0;
        }
      }
    }
  }
}

bool lk_sizes_ok(int64_t nimg, int64_t rows, int64_t cols, int64_t levels) {
  return nimg >= 0 && nimg <= 65535 && rows >= 1 && cols >= 1 && rows <= 16384 && cols <= 16384 && levels >= 1 &&
         levels <= kLkMaxLevels && nimg * rows * cols < ((int64_t)1 << 40);
}

// cyclic columns: every level in use is one period, level l has exactly cols >> l columns
bool lk_cyclic_cols_ok(int64_t cols, int64_t levels) { return cols % ((int64_t)1 << (levels - 1)) == 0; }

// the levels of a frame store's images as the kernels' table
LkLevels lk_store_levels(const sosvo_lk_images& im) {
  LkLevels t;
  int rows = im.rows, cols = im.cols;
  for (int l = 0; l < kLkMaxLevels; ++l) {
    t.base[l] = im.level[l];
    t.rows[l] = rows;
    t.cols[l] = cols;
    rows = (rows + 1) / 2;
    cols = (cols + 1) / 2;
  }
  return t;
}

// the levels 1 .. levels - 1 of all nimg images of the table, each from the one below
int32_t lk_build_levels(sosvo_ctx* ctx, const LkLevels& t, int nimg, int levels, const int32_t* row_range, bool cyclic = false) {
  for (int l = 0; l + 1 < levels; ++l) {
    const dim3 grid(cdiv(t.cols[l + 1], kPyrTileX), cdiv(t.rows[l + 1], kPyrTileY), nimg);
    SOSVO_LAUNCH_AS(ctx, cyclic ? "lk_pyr_down_cyclic_kernel" : "lk_pyr_down_kernel", cyclic ? lk_pyr_down_cyclic_kernel : lk_pyr_down_kernel,
                    grid, dim3(kPyrTileX, kPyrTileY), 0, ctx->stream, t.base[l], t.rows[l], t.cols[l], const_cast<uint8_t*>(t.base[l + 1]),
                    t.rows[l + 1], t.cols[l + 1], row_range, nimg > 1 ? nimg / 2 : 1, t.rows[0], l);
    SOSVO_LAUNCH_CHECK(ctx);
  }
  return SOSVO_OK;
}

// the tracker's arguments over a levels table, in LkArgs's member order (fb_max2, the last: lk_launch sets it per pass)
LkArgs lk_args(const LkLevels& lv, int nimg, int levels, int cap, int half, int max_iter, double eps, double min_eig, int initial_flow) {
  return LkArgs{lv, nimg, levels, cap, half, max_iter, initial_flow, eps * eps, min_eig, -1.0};
}

// sosvo_gray_pyramid and sosvo_gray_pyramid_cyclic
int32_t gray_pyramid(sosvo_ctx* ctx, const char* fn, bool cyclic, const uint8_t* gray, int32_t nimg, int32_t rows, int32_t cols,
                     int32_t levels, const int32_t* row_range, uint8_t* pyr) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE_FN(ctx, gray, "null pointer");
  SOSVO_REQUIRE_FN(ctx, lk_sizes_ok(nimg, rows, cols, levels), "sizes out of range (levels 1..4, rows and cols 1..16384)");
  SOSVO_REQUIRE_FN(ctx, !cyclic || lk_cyclic_cols_ok(cols, levels), "cyclic columns need cols to be a multiple of 2^(levels - 1)");
  SOSVO_REQUIRE_FN(ctx, pyr || levels == 1, "null pointer");
  SOSVO_REQUIRE_FN(ctx, row_range == nullptr || nimg % 2 == 0, "row_range needs the two views' images (nimg even, view-major)");
  if (nimg == 0) return SOSVO_OK;
  LkLevels t;
  lk_levels(gray, pyr, nimg, rows, cols, levels, &t);
  return lk_build_levels(ctx, t, nimg, levels, row_range, cyclic);
}

// the forward launch and, with `back`, the backward one (a: everything but initial_flow's reset and fb_max2, set here)
int32_t lk_launch(sosvo_ctx* ctx, LkArgs a, const int32_t* row_range, const int32_t* prev_img, const int32_t* next_img, int nprob,
                  const float* prev_pts, const int64_t* store_pt, const int32_t* n, float* next_pts, uint8_t* status, float* err,
                  float* back, double fb_max, bool cyclic = false) {
  a.fb_max2 = -1.0;
  const bool small = a.half <= 5;
  const int kpw = small ? 4 : 1;
  // waves per problem: enough for the chip at a few problems, several rounds per wave at thousands
  const dim3 grid(nprob, min(cdiv(a.cap, kpw), nprob >= 4096 ? 16 : 64));
  // (the profile labels a launch with its instantiation, as SOSVO_LAUNCH does)
  auto launch = [&](auto kernel, const char* name, const int32_t* from, const int32_t* to, const float* start, float* out, float* e,
                    const float* ref) {
    SOSVO_LAUNCH_AS(ctx, name, kernel, grid, dim3(64), 0, ctx->stream, a, row_range, from, to, start, n, out, status, e, ref, store_pt);
  };
  auto pass = [&](const int32_t* from, const int32_t* to, const float* start, float* out, float* e, const float* ref) {
    if (cyclic) {
      if (small) launch(lk_track_kernel<16, true>, "(lk_track_kernel<16, true>)", from, to, start, out, e, ref);
      else launch(lk_track_kernel<64, true>, "(lk_track_kernel<64, true>)", from, to, start, out, e, ref);
    } else {
      if (small) launch(lk_track_kernel<16>, "lk_track_kernel<16>", from, to, start, out, e, ref);
      else launch(lk_track_kernel<64>, "lk_track_kernel<64>", from, to, start, out, e, ref);
    }
  };
  pass(prev_img, next_img, prev_pts, next_pts, err, nullptr);
  SOSVO_LAUNCH_CHECK(ctx);
  if (back) {  // the forward results tracked back: images swapped, no initial guess
    a.initial_flow = 0;
    a.fb_max2 = fb_max * fb_max;
    pass(next_img, prev_img, next_pts, back, nullptr, prev_pts);
    SOSVO_LAUNCH_CHECK(ctx);
  }
  return SOSVO_OK;
}

// ---- static stereo by tracking (sosvo_refine_stereo_lk) ---------------------------------------------------
// The tracker above does the work; the new device code is the GATHER in front of it and the ACCEPTANCE behind it.
//
// Gather, one workgroup per problem p = frame * nmask + mask: the matched bottom keypoints that pass the pre-gate and have
// finite coordinates are COMPACTED into the tracker's tables -- start[p, j] = the top partner, guess[p, j] = the bottom
// keypoint, idx[p, j] = its row q -- so that no group of the tracker idles on a row that is not tracked; count[p] = how many,
// from[p] / to[p] = the frame's top / bottom image.  status[p, q] = 0 for every q < n_bot[p].  (The order inside a problem is
// that of q; it does not matter: the bottom rows are distinct.)
struct StereoLkGate {
  double max_du, min_dv, max_shift;  // max_du = +inf: the du side is off
  int dv_on;
};
constexpr double kStereoLkSlack = 1.0 / 1099511627776.0;  // 2^-40: far above the 2^-53 rounding of a difference, far below a pixel

__global__ __launch_bounds__(256) void stereo_lk_gather_kernel(int nmask, int nframes, int cap, const float* __restrict__ kp_top,
                                                               const int32_t* __restrict__ n_top, const float* __restrict__ kp_bot,
                                                               const int32_t* __restrict__ n_bot, const uint32_t* __restrict__ keys,
                                                               StereoLkGate g, float* __restrict__ start, float* __restrict__ guess,
                                                               int32_t* __restrict__ idx, int32_t* __restrict__ count,
                                                               int32_t* __restrict__ from, int32_t* __restrict__ to,
                                                               uint8_t* __restrict__ status) {
  __shared__ int wave_off[5];
  __shared__ int s_running;
  const int p = blockIdx.x, tid = threadIdx.x;
  const int nb = min(max(n_bot[p], 0), cap), nt = min(max(n_top[p], 0), cap);
  if (tid == 0) s_running = 0;
  __syncthreads();
  const size_t base = (size_t)p * cap;
  for (int q0 = 0; q0 < nb; q0 += 256) {  // (uniform)
    const int q = q0 + tid;
    bool track = false;
    float ut = 0.f, vt = 0.f, ub = 0.f, vb = 0.f;
    if (q < nb) {
      if (status) status[base + q] = 0;
      const uint32_t key = keys[base + q];
      const int t = (int)(key & SOSVO_KEY_IDX_MASK);
      if (key != SOSVO_KEY_NONE && t < nt) {
        ut = kp_top[2 * (base + t)];
        vt = kp_top[2 * (base + t) + 1];
        ub = kp_bot[2 * (base + q)];
        vb = kp_bot[2 * (base + q) + 1];
        const double du = (double)ut - (double)ub, dv = (double)vt - (double)vb;
        // the pre-gate (a NaN difference compares false: the pair goes on and fails the test below)
        const bool far_u = fabs(du) > (g.max_du + g.max_shift) * (1.0 + kStereoLkSlack);
        const bool far_v = g.dv_on && dv + g.max_shift < g.min_dv - kStereoLkSlack * (fabs(dv) + g.max_shift + g.min_dv);
        track = !far_u && !far_v && isfinite(ut) && isfinite(vt) && isfinite(ub) && isfinite(vb);
      }
    }
    const int pos = sosvo_block_compact_pos<4>(track, wave_off, &s_running, tid);
    if (track) {  // (pos < nb <= cap)
      start[2 * (base + pos)] = ut;
      start[2 * (base + pos) + 1] = vt;
      guess[2 * (base + pos)] = ub;
      guess[2 * (base + pos) + 1] = vb;
      idx[base + pos] = q;
    }
  }
  __syncthreads();
  if (tid == 0) {
    count[p] = s_running;
    from[p] = p / nmask;
    to[p] = nframes + p / nmask;
  }
}

// Acceptance: entry j < count[p] of problem p is the bottom row q = idx[p, j]; kp_bot[p, q] still holds the guess.  The
// tracked position replaces it iff the tracker's status is 1 and it lies within max_shift of the guess on both axes (float32
// values compared in double; a NaN fails).
__global__ __launch_bounds__(256) void stereo_lk_accept_kernel(int nprob, int cap, double max_shift, const int32_t* __restrict__ count,
                                                               const int32_t* __restrict__ idx, const float* __restrict__ next,
                                                               const uint8_t* __restrict__ tracked, float* __restrict__ kp_bot,
                                                               uint8_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)nprob * cap) return;
  const int p = (int)(i / cap), j = (int)(i - (size_t)p * cap);
  if (j >= min(count[p], cap) || tracked[i] == 0) return;
  const int q = idx[i];
  if (q < 0 || q >= cap) return;  // (never: the gather wrote it)
  const size_t o = (size_t)p * cap + q;
  const float x = next[2 * i], y = next[2 * i + 1];
  const double dx = (double)x - (double)kp_bot[2 * o], dy = (double)y - (double)kp_bot[2 * o + 1];
  if (!(fabs(dx) <= max_shift && fabs(dy) <= max_shift)) return;
  kp_bot[2 * o] = x;
  kp_bot[2 * o + 1] = y;
  if (status) status[o] = 1;
}

}  // namespace

bool sosvo_stereo_lk_options_ok(const sosvo_stereo_lk_options& o) {
  return o.half >= 2 && o.half <= kLkMaxHalf && o.max_iter >= 1 && o.max_iter <= 30 && o.eps >= 0.0 && isfinite(o.eps) &&
         o.min_eig >= 0.0 && isfinite(o.min_eig) && o.max_shift >= 0.0 && isfinite(o.max_shift);
}

bool sosvo_lk_options_ok(const sosvo_lk_options& o) {
  return o.half >= 2 && o.half <= kLkMaxHalf && o.levels >= 1 && o.levels <= kLkMaxLevels && o.max_iter >= 1 && o.max_iter <= 30 &&
         o.eps >= 0.0 && isfinite(o.eps) && o.min_eig >= 0.0 && isfinite(o.min_eig) && isfinite(o.fb_max);
}

// (internal, common.h) The images of nframes frames into a frame store.  gray [2, nframes, rows, cols]: the front end's gray
// rows, frame i goes to slot slot_of_frame[i] (HOST table, checked by the caller) or first_slot + i; gray == nullptr: level 0 of
// the store IS the front end's buffer (a pair batch, frame i in slot i) and nothing is copied.  Then the levels in use, each
// from the one below inside the store.  The table travels in kernel arguments, kSosvoSlotArgFrames frames per launch.
// pad > 0: gray is [2, nframes, rows, cols + 2 pad], the rows of a padded front end, and level 0 takes their interior.
int32_t sosvo_lk_images_fill(sosvo_ctx* ctx, const sosvo_lk_images& im, int32_t levels, const int32_t* row_range, const uint8_t* gray,
                             int32_t nframes, int32_t first_slot, const int32_t* slot_of_frame, bool cyclic, int32_t pad) {
  SOSVO_REQUIRE(ctx, im.level[0] && im.level[1] && im.level[2] && im.level[3], "null pointer");
  SOSVO_REQUIRE(ctx, lk_sizes_ok(2 * (int64_t)im.slots, im.rows, im.cols, levels), "sizes out of range (2 * slots <= 65535, levels 1..4)");
  const LkLevels t = lk_store_levels(im);
  SOSVO_REQUIRE(ctx, !cyclic || lk_cyclic_cols_ok(im.cols, levels), "cyclic columns need cols to be a multiple of 2^(levels - 1)");
  if (!gray) return lk_build_levels(ctx, t, 2 * im.slots, levels, row_range, cyclic);
  for (int f0 = 0; f0 < nframes; f0 += kSosvoSlotArgFrames) {
    const int nf = nframes - f0 < kSosvoSlotArgFrames ? nframes - f0 : kSosvoSlotArgFrames;
    sosvo_slot_table tab;
    for (int i = 0; i < kSosvoSlotArgFrames; ++i) tab.slot[i] = i >= nf ? 0 : slot_of_frame ? slot_of_frame[f0 + i] : first_slot + f0 + i;
    for (int i = 0; i < nf; ++i) SOSVO_REQUIRE(ctx, tab.slot[i] >= 0 && tab.slot[i] < im.slots, "slot out of range");
    const int blocks = min(cdiv(im.rows * im.cols, 4096), 64);
    if (pad > 0)
      SOSVO_LAUNCH(ctx, lk_store_level0_padded_kernel, dim3(blocks, nf, 2), dim3(256), 0, ctx->stream, gray, nframes, f0, tab, im.slots,
                   im.rows, im.cols, pad, row_range, im.level[0]);
    else
      SOSVO_LAUNCH(ctx, lk_store_level0_kernel, dim3(blocks, nf, 2), dim3(256), 0, ctx->stream, gray, nframes, f0, tab, im.slots, im.rows,
                   im.cols, row_range, im.level[0]);
    SOSVO_LAUNCH_CHECK(ctx);
    for (int l = 0; l + 1 < levels; ++l) {
      const dim3 grid(cdiv(t.cols[l + 1], kPyrTileX), cdiv(t.rows[l + 1], kPyrTileY), 2 * nf);
      SOSVO_LAUNCH_AS(ctx, cyclic ? "lk_pyr_down_slots_cyclic_kernel" : "lk_pyr_down_slots_kernel",
                      cyclic ? lk_pyr_down_slots_cyclic_kernel : lk_pyr_down_slots_kernel, grid, dim3(kPyrTileX, kPyrTileY), 0, ctx->stream,
                      t.base[l], t.rows[l], t.cols[l], im.level[l + 1], t.rows[l + 1], t.cols[l + 1], row_range, nf, tab, im.slots, im.rows, l);
      SOSVO_LAUNCH_CHECK(ctx);
    }
  }
  return SOSVO_OK;
}

// (internal, common.h) sosvo_track_lk on a frame store's images with the settings o: problem p tracks the n[p] points that lie
// from point store_pt[p] of `pts` on (DEVICE table; points, not floats) from image from_img[p] to image to_img[p]; outputs as
// sosvo_track_lk's, [nprob, cap, ...]; back: its buffer, used when o.fb_max > 0.
int32_t sosvo_lk_images_track(sosvo_ctx* ctx, const sosvo_lk_images& im, const sosvo_lk_options& o, const int32_t* row_range,
                              const int32_t* from_img, const int32_t* to_img, int32_t nprob, int32_t cap, const float* pts,
                              const int64_t* store_pt, const int32_t* n, float* next_pts, uint8_t* status, float* err, float* back,
                              bool cyclic) {
  SOSVO_REQUIRE(ctx, im.level[0] && im.level[1] && im.level[2] && im.level[3] && from_img && to_img && pts && store_pt && n &&
                         next_pts && status && err && back,
                "null pointer");
  SOSVO_REQUIRE(ctx, sosvo_lk_options_ok(o), "LK settings out of range (sosvo_set_lk_options)");
  SOSVO_REQUIRE(ctx, lk_sizes_ok(2 * (int64_t)im.slots, im.rows, im.cols, o.levels), "sizes out of range (2 * slots <= 65535)");
  SOSVO_REQUIRE(ctx, nprob >= 0 && nprob <= 65535 && cap > 0, "nprob / cap out of range");
  SOSVO_REQUIRE(ctx, !cyclic || (lk_cyclic_cols_ok(im.cols, o.levels) && (im.cols >> (o.levels - 1)) >= 2 * o.half + 3),
                "cyclic columns need cols % 2^(levels - 1) == 0 and 2 half + 3 columns on the top level");
  if (nprob == 0) return SOSVO_OK;
  LkLevels t = lk_store_levels(im);
  for (int l = o.levels; l < kLkMaxLevels; ++l) t.base[l] = nullptr;  // (not built, never read)
  const LkArgs a = lk_args(t, 2 * im.slots, o.levels, cap, o.half, o.max_iter, o.eps, o.min_eig, 0);
  return lk_launch(ctx, a, row_range, from_img, to_img, nprob, pts, store_pt, n, next_pts, status, err, o.fb_max > 0.0 ? back : nullptr,
                   o.fb_max, cyclic);
}

extern "C" {

int32_t sosvo_gray_pyramid_bytes(sosvo_ctx* ctx, int32_t nimg, int32_t rows, int32_t cols, int32_t levels, int64_t* bytes) {
  if (!bytes) return sosvo_fail(ctx, SOSVO_ERR_ARG, __func__, "null pointer");
  if (!lk_sizes_ok(nimg, rows, cols, levels)) return sosvo_fail(ctx, SOSVO_ERR_ARG, __func__, "sizes out of range (levels 1..4)");
  *bytes = lk_levels(nullptr, nullptr, nimg, rows, cols, levels, nullptr);
  return SOSVO_OK;
}

int32_t sosvo_gray_pyramid(sosvo_ctx* ctx, const uint8_t* gray, int32_t nimg, int32_t rows, int32_t cols, int32_t levels,
                           const int32_t* row_range, uint8_t* pyr) {
  return gray_pyramid(ctx, __func__, false, gray, nimg, rows, cols, levels, row_range, pyr);
}

int32_t sosvo_gray_pyramid_cyclic(sosvo_ctx* ctx, const uint8_t* gray, int32_t nimg, int32_t rows, int32_t cols, int32_t levels,
                                  const int32_t* row_range, uint8_t* pyr) {
  return gray_pyramid(ctx, __func__, true, gray, nimg, rows, cols, levels, row_range, pyr);
}

int32_t sosvo_track_lk(sosvo_ctx* ctx, const uint8_t* gray, const uint8_t* pyr, int32_t nimg, int32_t rows, int32_t cols,
                       int32_t levels, const int32_t* row_range, const int32_t* prev_img, const int32_t* next_img, int32_t nprob,
                       int32_t cap, const float* prev_pts, const int32_t* n, int32_t half, int32_t max_iter, double eps,
                       double min_eig, int32_t flags, float* next_pts, uint8_t* status, float* err, float* back, double fb_max) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, gray && prev_img && next_img && prev_pts && n && next_pts && status && err, "null pointer");
  SOSVO_REQUIRE(ctx, lk_sizes_ok(nimg, rows, cols, levels), "sizes out of range (levels 1..4, rows and cols 1..16384)");
  SOSVO_REQUIRE(ctx, pyr || levels == 1, "null pointer (the levels above 0)");
  SOSVO_REQUIRE(ctx, row_range == nullptr || nimg % 2 == 0, "row_range needs the two views' images (nimg even, view-major)");
  SOSVO_REQUIRE(ctx, nprob >= 0 && nprob <= 65535, "nprob out of range");
  SOSVO_REQUIRE(ctx, cap > 0 && cap <= 4096, "cap out of range");
  SOSVO_REQUIRE(ctx, half >= 2 && half <= kLkMaxHalf, "half out of range (2..10)");
  SOSVO_REQUIRE(ctx, max_iter >= 1 && max_iter <= 30, "max_iter out of range (1..30)");
  SOSVO_REQUIRE(ctx, eps >= 0.0 && min_eig >= 0.0, "eps / min_eig must not be negative or NaN");
  SOSVO_REQUIRE(ctx, (flags & ~(SOSVO_LK_INITIAL_FLOW | SOSVO_LK_CYCLIC_COLUMNS)) == 0, "unknown flag");
  const bool cyclic = (flags & SOSVO_LK_CYCLIC_COLUMNS) != 0;
  SOSVO_REQUIRE(ctx, !cyclic || lk_cyclic_cols_ok(cols, levels), "cyclic columns need cols to be a multiple of 2^(levels - 1)");
  SOSVO_REQUIRE(ctx, !cyclic || (cols >> (levels - 1)) >= 2 * half + 3,
                "cyclic columns need 2 half + 3 columns on the top level (the template fits one period)");
  SOSVO_REQUIRE(ctx, back == nullptr || fb_max > 0.0, "fb_max must be positive with a back buffer");
  if (nprob == 0 || nimg == 0) return SOSVO_OK;
  LkLevels t;
  lk_levels(gray, pyr, nimg, rows, cols, levels, &t);
  const LkArgs a = lk_args(t, nimg, levels, cap, half, max_iter, eps, min_eig, (flags & SOSVO_LK_INITIAL_FLOW) ? 1 : 0);
  return lk_launch(ctx, a, row_range, prev_img, next_img, nprob, prev_pts, nullptr, n, next_pts, status, err, back, fb_max, cyclic);
}

int32_t sosvo_refine_stereo_lk(sosvo_ctx* ctx, const uint8_t* gray, int32_t nimg, int32_t rows, int32_t cols,
                               const int32_t* row_range, int32_t nmask, int32_t cap, const float* kp_top, const int32_t* n_top,
                               float* kp_bot, const int32_t* n_bot, const uint32_t* keys, double stereo_min_disp,
                               double stereo_max_hdiff, const sosvo_stereo_lk_options* options, uint8_t* status) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, gray && kp_top && n_top && kp_bot && n_bot && keys, "null pointer");
  SOSVO_REQUIRE(ctx, lk_sizes_ok(nimg, rows, cols, 1) && nimg % 2 == 0, "sizes out of range (nimg even: view-major top / bottom images)");
  SOSVO_REQUIRE(ctx, nmask >= 1 && cap > 0 && cap <= 4096 && (int64_t)(nimg / 2) * nmask <= 65535, "nmask / cap / problem count out of range");
  const sosvo_stereo_lk_options o = options ? *options : ctx->stereo_lk;
  SOSVO_REQUIRE(ctx, sosvo_stereo_lk_options_ok(o),
                "settings out of range: half 2..10, max_iter 1..30, eps and min_eig finite and >= 0, max_shift finite and >= 0");
  SOSVO_REQUIRE(ctx, !isnan(stereo_min_disp) && !isnan(stereo_max_hdiff), "the gates must not be NaN");
  const int F = nimg / 2, P = F * nmask;
  if (P == 0) return SOSVO_OK;
  // the tracker's tables, in the context's scratch
  const size_t n_pts = (size_t)P * cap;
  float *start, *next, *err;
  int32_t *idx, *count, *from, *to;
  uint8_t* tracked;
  int32_t rc = sosvo_ws_carve(ctx, [&](Carver& cv) {
    start = cv.take<float>(2 * n_pts);
    next = cv.take<float>(2 * n_pts);
    err = cv.take<float>(n_pts);
    idx = cv.take<int32_t>(n_pts);
    tracked = cv.take<uint8_t>(n_pts);
    count = cv.take<int32_t>(P);
    from = cv.take<int32_t>(P);
    to = cv.take<int32_t>(P);
  });
  if (rc != SOSVO_OK) return rc;
  const double max_shift = o.max_shift > 0.0 ? o.max_shift : (double)o.half;
  StereoLkGate g;  // sv_pixel_gate's switches: the du side is on for max_hdiff > 0, the dv side for min_disp >= 0
  g.max_du = stereo_max_hdiff > 0 ? stereo_max_hdiff : HUGE_VAL;
  g.dv_on = stereo_min_disp >= 0 ? 1 : 0;
  g.min_dv = g.dv_on ? stereo_min_disp : 0.0;
  g.max_shift = max_shift;
  SOSVO_LAUNCH(ctx, stereo_lk_gather_kernel, dim3(P), dim3(256), 0, ctx->stream, nmask, F, cap, kp_top, n_top, kp_bot, n_bot, keys, g,
               start, next, idx, count, from, to, status);
  SOSVO_LAUNCH_CHECK(ctx);
  LkLevels t;
  lk_levels(gray, nullptr, nimg, rows, cols, 1, &t);
  const LkArgs a = lk_args(t, nimg, 1, cap, o.half, o.max_iter, o.eps, o.min_eig, 1);
  rc = lk_launch(ctx, a, row_range, from, to, P, start, nullptr, count, next, tracked, err, nullptr, 0.0);
  if (rc != SOSVO_OK) return rc;
  SOSVO_LAUNCH(ctx, stereo_lk_accept_kernel, dim3((unsigned)((n_pts + 255) / 256)), dim3(256), 0, ctx->stream, P, cap, max_shift, count,
               idx, next, tracked, kp_bot, status);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

}  // extern "C"
