// Dense omnistereo: semi-global matching between the top and the bottom gray panorama of a coaxial
// rig, whose epipolar lines are the panorama's columns, and the triangulation of the resulting disparity map.
//   OmniStereoModel.get_depth_map_from_panoramas (camera_models.py:3395) with common_cv.StereoMatchTuner's SGBM settings
//   (common_cv.py:482-497, :644), resolve_pano_correspondences_from_disparity_map (:2492), triangulate_from_depth_map (:2567)
// The algorithm is the one include/sosvo.h states for sosvo_dense_stereo (tests/refdense.py is the same text in numpy):
// 9 x 7 census, Hamming cost over D = 64 disparities, four aggregation paths (eight with sosvo_dense_stereo_paths, DESIGN.md
// section 39, tests/refdense8.py), winner + uniqueness + left-right + 1/16-row parabola.  Small integers throughout, so the
// device equals the numpy statement bit for bit.
//
// Lane = disparity: a wave64 holds the 64 values L(p, .) of one pixel of one scan line.  The path minimum is four DPP
// exchanges inside the rows of 16 lanes and four readlanes; the k - 1 / k + 1 terms are the whole-wave shifts of common.h
// with the entering lane poisoned.  No LDS.  The cost volume C [n, rows, cols, 64] u8 is written once, by the downward
// pass (there the bottom column's census words slide one lane per row: one shift and one new word per step), and read
// by the other three passes as one 64-byte line per step; S [n, rows, cols, 64] u16 is written by the downward pass and
// added to by the other three (and by the four diagonal passes), one launch after the other on the context's stream.
#include "common.h"
#include "dense_scratch.h"
#include "geom_core.h"

namespace {

constexpr int kD = 64;              // disparities = lanes
constexpr int kBig = 1 << 20;       // above any L (<= 64 + 8191) plus P1
constexpr uint32_t kRowBits = 14;   // rows <= 16384: a row index fits 14 bits of the left-right key

// L(p, k) = C(p, k) + min(L_prev(k), L_prev(k - 1) + P1, L_prev(k + 1) + P1, m + P2) - m, m = min_j L_prev(j)
__device__ __forceinline__ int sgm_step(int cost, int Lp, int P1, int P2, int lane) {
  const int m = wave_min(Lp);
  int a = lane_from_left(Lp), b = lane_from_right(Lp);
  a = lane == 0 ? kBig : a;        // a missing neighbour does not take part
  b = lane == kD - 1 ? kBig : b;
  return cost + min(min(Lp, m + P2), min(a, b) + P1) - m;
}

// census [nimg, rows, cols] u64 of gray [nimg, rows, cols] u8: one lane per pixel.  Rows clamp; columns clamp or wrap.
template <bool kCyclic>
__global__ __launch_bounds__(256) void dense_census_kernel(const uint8_t* __restrict__ gray, int rows, int cols,
                                                           uint64_t* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  const size_t line = blockIdx.y + (size_t)blockIdx.z * gridDim.y;  // img * rows + r
  const int r = (int)(line % (size_t)rows);
  const uint8_t* img = gray + (line - r) * cols;
  int cc[7];
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    int x = c + j - 3;
    if (kCyclic) {  // (a loop only where the image is narrower than the window's reach)
      while (x < 0) x += cols;
      while (x >= cols) x -= cols;
    } else {
      x = clampi(x, 0, cols - 1);
    }
    cc[j] = x;
  }
  const int centre = img[(size_t)r * cols + c];
  uint64_t w = 0;
#pragma unroll
  for (int dy = -4; dy <= 4; ++dy) {
    const uint8_t* row = img + (size_t)clampi(r + dy, 0, rows - 1) * cols;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      if (dy == 0 && j == 3) continue;
      w = (w << 1) | (uint64_t)((int)row[cc[j]] < centre);
    }
  }
  out[line * cols + c] = w;
}

// The downward path of column c of frame f (one wave): the costs from the census words, C and S = L written.
__global__ __launch_bounds__(256) void dense_down_kernel(const uint64_t* __restrict__ census_top, const uint64_t* __restrict__ census_bot,
                                                         int rows, int cols, int d0, int P1, int P2, uint8_t* __restrict__ C,
                                                         uint16_t* __restrict__ S) {
  const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= cols) return;  // (the whole wave)
  const size_t frame = (size_t)blockIdx.y * rows * cols;
  const uint64_t* ct = census_top + frame + c;
  const uint64_t* cb = census_bot + frame + c;
  uint32_t wlo = 0, whi = 0;  // the bottom word of row r - d0 - lane
  int Lp = 0;
  for (int r = 0; r < rows; ++r) {
    wlo = (uint32_t)lane_from_left((int)wlo);
    whi = (uint32_t)lane_from_left((int)whi);
    const int rb0 = r - d0;
    if (rb0 >= 0) {  // (uniform)
      const uint64_t nw = cb[(size_t)rb0 * cols];
      if (lane == 0) {
        wlo = (uint32_t)nw;
        whi = (uint32_t)(nw >> 32);
      }
    }
    const uint64_t t = ct[(size_t)r * cols];
    const int cost = rb0 - lane >= 0 ? __popc(wlo ^ (uint32_t)t) + __popc(whi ^ (uint32_t)(t >> 32)) : 64;
    const int L = r == 0 ? cost : sgm_step(cost, Lp, P1, P2, lane);
    const size_t i = (frame + (size_t)r * cols + c) * kD + lane;
    C[i] = (uint8_t)cost;
    S[i] = (uint16_t)L;
    Lp = L;
  }
}

// One further path per wave: line `l` of frame f starts at pixel base + l * line_stride and takes len steps of `step`
// pixels.  C is read, L is added to S.  The next step's C and S are in flight while this step's recurrence runs (eight steps
// ahead was tried: 190 to 304 VGPRs, one wave per SIMD, 2.4 to 6 times slower at n = 64 and no faster at n = 1).
__global__ __launch_bounds__(256) void dense_path_kernel(const uint8_t* __restrict__ C, uint16_t* __restrict__ S, int nlines, int len,
                                                         long long frame_pixels, long long base, long long line_stride,
                                                         long long step, int P1, int P2) {
  const int lane = threadIdx.x & 63, l = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (l >= nlines) return;  // (the whole wave)
  long long p = (long long)blockIdx.y * frame_pixels + base + (long long)l * line_stride;
  int cn = C[(size_t)p * kD + lane], sn = S[(size_t)p * kD + lane], Lp = 0;
  for (int i = 0; i < len; ++i) {
    const int cost = cn, s = sn;
    const long long q = p + step;
    if (i + 1 < len) {
      cn = C[(size_t)q * kD + lane];
      sn = S[(size_t)q * kD + lane];
    }
    const int L = i == 0 ? cost : sgm_step(cost, Lp, P1, P2, lane);
    S[(size_t)p * kD + lane] = (uint16_t)(s + L);
    Lp = L;
    p = q;
  }
}

// One diagonal path per wave: line j of frame f starts in column j of the first row (dr = +1) or of
// the last row (dr = -1) and at every step moves one row by dr and one column by dc, the column wrapping modulo cols, so that
// the cols lines of a launch visit every pixel exactly once.  Cyclic: the wrap is the predecessor across the seam.  Clamped:
// the line starts again with L = C in the column it wraps into.  The wave's number is made uniform, so the pixel, its column
// and the wrap are scalar; C, S and the one-step-ahead loads are those of dense_path_kernel.  One direction per launch: two
// of them in one launch would have two waves read-modify-write the same S.
template <bool kCyclic>
__global__ __launch_bounds__(256) void dense_diag_kernel(const uint8_t* __restrict__ C, uint16_t* __restrict__ S, int rows, int cols, int dr,
                                                         int dc, int P1, int P2) {
  const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (j >= cols) return;  // (the whole wave)
  const long long row_step = dr > 0 ? (long long)cols : -(long long)cols;
  const int start_col = dc > 0 ? 0 : cols - 1;  // clamped: where a line starts again
  long long p = (long long)blockIdx.y * rows * cols + (dr > 0 ? 0LL : (long long)(rows - 1) * cols) + j;
  int c = j, cn = C[(size_t)p * kD + lane], sn = S[(size_t)p * kD + lane], Lp = 0;
  for (int i = 0; i < rows; ++i) {
    const int cost = cn, s = sn;
    int c2 = c + dc;
    long long q = p + row_step + dc;
    if (c2 == cols) {
      c2 = 0;
      q -= cols;
    } else if (c2 < 0) {
      c2 = cols - 1;
      q += cols;
    }
    if (i + 1 < rows) {
      cn = C[(size_t)q * kD + lane];
      sn = S[(size_t)q * kD + lane];
    }
    const int L = i == 0 || (!kCyclic && c == start_col) ? cost : sgm_step(cost, Lp, P1, P2, lane);
    S[(size_t)p * kD + lane] = (uint16_t)(s + L);
    Lp = L;
    p = q;
    c = c2;
  }
}

// Winner, uniqueness, reach, mask and the parabola of 64 consecutive pixels per wave; d16 before the left-right check,
// kstar (0xFF = dropped), and with `best` the left-right key (mS << 14 | r) of the bottom row the pixel points at.
// First lane = disparity, one pixel after the other: the reductions (winner key, rivals, the two neighbours of the winner),
// whose results lane j keeps for pixel j.  Then lane = pixel: tests, the parabola's division and the stores once per pixel
// (with one wave per pixel through to the stores the kernel was bound by the VALU, all 64 lanes dividing for one pixel).
__global__ __launch_bounds__(256) void dense_select_kernel(const uint16_t* __restrict__ S, const uint8_t* __restrict__ mask, int rows, int cols,
                                                           size_t total, int d0, int uniqueness, int16_t* __restrict__ d16,
                                                           uint8_t* __restrict__ kstar, uint32_t* __restrict__ best) {
  const int lane = threadIdx.x & 63;
  const size_t first = ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * kD, frame_pixels = (size_t)rows * cols;
  if (first >= total) return;  // (the whole wave)
  const int count = (int)min((size_t)kD, total - first);
  int my_key = 0, my_a = 0, my_b = 0, my_rival = 0;
  for (int j0 = 0; j0 < count; j0 += 8) {
    int sv[8];  // (eight pixels' loads in flight before the first reduction; pixels beyond `count` read as 0 and are not kept)
#pragma unroll
    for (int i = 0; i < 8; ++i) sv[i] = j0 + i < count ? S[(first + j0 + i) * kD + lane] : 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int s = sv[i];
      const int key = wave_min((s << 6) | lane);  // the smallest k among the minimal S
      const int ks = key & 63, mS = key >> 6;
      const bool rival = abs(lane - ks) > 1 && s * (100 - uniqueness) < mS * 100;
      const int any = __ballot(rival) != 0ULL ? 1 : 0;
      const int a = __shfl(s, max(ks - 1, 0)), b = __shfl(s, min(ks + 1, kD - 1));
      if (lane == j0 + i) {
        my_key = key;
        my_a = a;
        my_b = b;
        my_rival = any;
      }
    }
  }
  if (lane >= count) return;
  const size_t p = first + lane, pix = p % frame_pixels;
  const int ks = my_key & 63, mS = my_key >> 6;
  const int r = (int)(pix / cols), rb = r - (d0 + ks);
  const bool drop = my_rival != 0 || rb < 0 || (mask && mask[pix] == 0);
  int off = 0;
  if (ks >= 1 && ks <= kD - 2) {
    const int den = max(my_a + my_b - 2 * mS, 1), num = (my_a - my_b) * 16 + den;
    off = num >= 0 ? num / (2 * den) : -((-num + 2 * den - 1) / (2 * den));  // floor
  }
  d16[p] = drop ? (int16_t)-1 : (int16_t)((d0 + ks) * 16 + off);
  kstar[p] = drop ? (uint8_t)0xFF : (uint8_t)ks;
  if (best && !drop) atomicMin(best + (p - pix) + (size_t)rb * cols + (pix - (size_t)r * cols), ((uint32_t)mS << kRowBits) | (uint32_t)r);
}

// Left-right: a surviving pixel goes where the pixel kept by its bottom row has a k* further than lr_max from its own.
__global__ __launch_bounds__(256) void dense_left_right_kernel(const uint8_t* __restrict__ kstar, const uint32_t* __restrict__ best, int rows,
                                                               int cols, size_t total, int d0, int lr_max, int16_t* __restrict__ d16) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= total) return;
  const int ks = kstar[p];
  if (ks == 0xFF) return;
  const size_t frame_pixels = (size_t)rows * cols, pix = p % frame_pixels;
  const int r = (int)(pix / cols), c = (int)(pix - (size_t)r * cols), rb = r - (d0 + ks);
  const uint32_t key = best[(p - pix) + (size_t)rb * cols + c];  // (written by this pixel at the latest)
  const int kept = kstar[(p - pix) + (size_t)(key & ((1u << kRowBits) - 1)) * cols + c];
  if (abs(kept - ks) > lr_max) d16[p] = -1;
}

struct DenseRig {
  double pano_top[4], pano_bot[4], F_top[3], F_bot[3], min_range, max_range;
};

// One lane per pixel: top (c, r), bottom (c, r - d16 / 16) -> angles -> midpoint -> range, with the sparse path's functions.
__global__ __launch_bounds__(256) void dense_triangulate_kernel(DenseRig rig, const int16_t* __restrict__ d16, int rows, int cols,
                                                                size_t total, int min_d16, int max_d16, double* __restrict__ X) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= total) return;
  const int d = d16[p];
  double x[3] = {sv_nan(), sv_nan(), sv_nan()};
  if (d >= 0 && d >= min_d16 && (max_d16 <= 0 || d <= max_d16)) {
    const size_t pix = p % ((size_t)rows * cols);
    const int r = (int)(pix / cols), c = (int)(pix - (size_t)r * cols);
    double az1, el1, az2, el2, t[3];
    sv_pano_angles((double)c, (double)r, rig.pano_top, &az1, &el1);
    sv_pano_angles((double)c, (double)r - (double)d / 16.0, rig.pano_bot, &az2, &el2);
    sv_triangulate(az1, el1, az2, el2, rig.F_top, rig.F_bot, t);
    if (sv_range_ok(t, rig.min_range, rig.max_range)) {
      x[0] = t[0];
      x[1] = t[1];
      x[2] = t[2];
    }
  }
  X[3 * p] = x[0];
  X[3 * p + 1] = x[1];
  X[3 * p + 2] = x[2];
}

int32_t launch_census(sosvo_ctx* ctx, const uint8_t* gray, int nimg, int rows, int cols, bool cyclic, uint64_t* out) {
  const dim3 grid(cdiv(cols, 256), rows, nimg);
  if (cyclic)
    SOSVO_LAUNCH(ctx, dense_census_kernel<true>, grid, dim3(256), 0, ctx->stream, gray, rows, cols, out);
  else
    SOSVO_LAUNCH(ctx, dense_census_kernel<false>, grid, dim3(256), 0, ctx->stream, gray, rows, cols, out);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

// What sosvo_dense_stereo, sosvo_dense_stereo_paths and sosvo_dense_stereo_wide (dense_wide.hip) refuse alike, in this order
int32_t dense_stereo_check(const char* fn, sosvo_ctx* ctx, const uint8_t* top, const uint8_t* bot, int32_t n, int32_t rows, int32_t cols,
                           int32_t min_disparity, int32_t P1, int32_t P2, int32_t uniqueness, int32_t flags, int32_t paths,
                           const int16_t* d16_out) {
  SOSVO_REQUIRE_FN(ctx, top && bot && d16_out, "null pointer");
  SOSVO_REQUIRE_DENSE_SIZE_AS(SOSVO_REQUIRE_FN, ctx, rows, cols);
  SOSVO_REQUIRE_DENSE_N_AS(SOSVO_REQUIRE_FN, ctx, n);
  SOSVO_REQUIRE_FN(ctx, P1 >= 0 && P1 <= P2 && P2 <= 8191, "penalties out of range (0 <= P1 <= P2 <= 8191)");
  SOSVO_REQUIRE_FN(ctx, uniqueness >= 0 && uniqueness < 100, "uniqueness out of range (0..99)");
  SOSVO_REQUIRE_FN(ctx, min_disparity >= 0 && min_disparity <= 1024, "min_disparity out of range (0..1024)");
  SOSVO_REQUIRE_DENSE_FLAGS_AS(SOSVO_REQUIRE_FN, ctx, flags);
  SOSVO_REQUIRE_FN(ctx, paths == 4 || paths == 8, "paths must be 4 or 8");
  SOSVO_REQUIRE_FN(ctx, paths == 4 || P2 <= SOSVO_DENSE_MAX_P2_EIGHT_PATHS, "eight paths need P2 <= 8127 (S stays 16 bits)");
  return SOSVO_OK;
}

int32_t dense_stereo_run(sosvo_ctx* ctx, const uint8_t* top, const uint8_t* bot, int32_t n, int32_t rows, int32_t cols, const uint8_t* mask,
                         int32_t min_disparity, int32_t P1, int32_t P2, int32_t uniqueness, int32_t lr_max, int32_t flags, int32_t paths,
                         int16_t* d16_out, uint16_t* S_out);

// sosvo_dense_stereo (paths = 4) and sosvo_dense_stereo_paths: one body, `fn` the public name in the messages
int32_t dense_stereo_body(const char* fn, sosvo_ctx* ctx, const uint8_t* top, const uint8_t* bot, int32_t n, int32_t rows, int32_t cols,
                          const uint8_t* mask, int32_t min_disparity, int32_t P1, int32_t P2, int32_t uniqueness, int32_t lr_max,
                          int32_t flags, int32_t paths, int16_t* d16_out, uint16_t* S_out) {
  SOSVO_ENTER(ctx);
  const int32_t ok = dense_stereo_check(fn, ctx, top, bot, n, rows, cols, min_disparity, P1, P2, uniqueness, flags, paths, d16_out);
  if (ok != SOSVO_OK) return ok;
  return dense_stereo_run(ctx, top, bot, n, rows, cols, mask, min_disparity, P1, P2, uniqueness, lr_max, flags, paths, d16_out, S_out);
}

// The launches of sosvo_dense_stereo (paths = 4) and sosvo_dense_stereo_paths on checked arguments
int32_t dense_stereo_run(sosvo_ctx* ctx, const uint8_t* top, const uint8_t* bot, int32_t n, int32_t rows, int32_t cols, const uint8_t* mask,
                         int32_t min_disparity, int32_t P1, int32_t P2, int32_t uniqueness, int32_t lr_max, int32_t flags, int32_t paths,
                         int16_t* d16_out, uint16_t* S_out) {
  const bool cyclic = (flags & SOSVO_DENSE_CYCLIC_COLUMNS) != 0, want_lr = lr_max >= 0;
  const size_t frame_pixels = (size_t)rows * cols, total = (size_t)n * frame_pixels;
  sosvo_dense_scratch b;  // (dense_scratch.h)
  const int32_t rc = sosvo_ws_carve(ctx, [&](Carver& cv) { b = sosvo_dense_carve(cv, total, kD, S_out != nullptr, want_lr); });
  if (rc != SOSVO_OK) return rc;
  uint64_t *census_top = b.census_top, *census_bot = b.census_bot;
  uint8_t *C = b.C, *kstar = b.kstar;
  uint16_t* S = S_out ? S_out : b.S;
  uint32_t* best = want_lr ? b.best : nullptr;

  int32_t st = launch_census(ctx, top, n, rows, cols, cyclic, census_top);
  if (st != SOSVO_OK) return st;
  st = launch_census(ctx, bot, n, rows, cols, cyclic, census_bot);
  if (st != SOSVO_OK) return st;
  SOSVO_LAUNCH(ctx, dense_down_kernel, dim3(cdiv(cols, 4), n), dim3(256), 0, ctx->stream, census_top, census_bot, rows, cols,
               min_disparity, P1, P2, C, S);
  SOSVO_LAUNCH_CHECK(ctx);
  {  // up: column c from the last row
    SOSVO_PROFILE(ctx, "dense_path_kernel_up");
    hipLaunchKernelGGL(dense_path_kernel, dim3(cdiv(cols, 4), n), dim3(256), 0, ctx->stream, C, S, cols, rows, (long long)frame_pixels,
                       (long long)(rows - 1) * cols, 1LL, -(long long)cols, P1, P2);
  }
  SOSVO_LAUNCH_CHECK(ctx);
  {  // left to right: row r from column 0
    SOSVO_PROFILE(ctx, "dense_path_kernel_lr");
    hipLaunchKernelGGL(dense_path_kernel, dim3(cdiv(rows, 4), n), dim3(256), 0, ctx->stream, C, S, rows, cols, (long long)frame_pixels,
                       0LL, (long long)cols, 1LL, P1, P2);
  }
  SOSVO_LAUNCH_CHECK(ctx);
  {  // right to left: row r from the last column
    SOSVO_PROFILE(ctx, "dense_path_kernel_rl");
    hipLaunchKernelGGL(dense_path_kernel, dim3(cdiv(rows, 4), n), dim3(256), 0, ctx->stream, C, S, rows, cols, (long long)frame_pixels,
                       (long long)cols - 1, (long long)cols, -1LL, P1, P2);
  }
  SOSVO_LAUNCH_CHECK(ctx);
  if (paths == 8) {  // the diagonals: line j from column j of the first (dr = +1) or the last row, one direction per launch
    static const struct { const char* name; int dr, dc; } kDiag[4] = {{"dense_diag_kernel_dr", 1, 1}, {"dense_diag_kernel_dl", 1, -1},
                                                                      {"dense_diag_kernel_ur", -1, 1}, {"dense_diag_kernel_ul", -1, -1}};
    for (const auto& d : kDiag) {
      SOSVO_LAUNCH_AS(ctx, d.name, cyclic ? dense_diag_kernel<true> : dense_diag_kernel<false>, dim3(cdiv(cols, 4), n), dim3(256), 0,
                      ctx->stream, C, S, rows, cols, d.dr, d.dc, P1, P2);
      SOSVO_LAUNCH_CHECK(ctx);
    }
  }
  if (want_lr) SOSVO_HIP(ctx, hipMemsetAsync(best, 0xFF, total * 4, ctx->stream));
  const size_t select_blocks = (total + 4 * kD - 1) / (4 * kD);
  SOSVO_LAUNCH(ctx, dense_select_kernel, dim3((unsigned)select_blocks), dim3(256), 0, ctx->stream, S, mask, rows, cols, total,
               min_disparity, uniqueness, d16_out, kstar, best);
  SOSVO_LAUNCH_CHECK(ctx);
  if (want_lr) {
    SOSVO_LAUNCH(ctx, dense_left_right_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, kstar, best, rows, cols,
                 total, min_disparity, lr_max, d16_out);
    SOSVO_LAUNCH_CHECK(ctx);
  }
  return SOSVO_OK;
}

}  // namespace

// For dense_wide.hip (declared in common.h): the shared refusals, the census launch, and the 64-disparity launches on checked arguments
int32_t sosvo_dense_stereo_check(const char* fn, sosvo_ctx* ctx, const uint8_t* top, const uint8_t* bot, int32_t n, int32_t rows,
                                 int32_t cols, int32_t min_disparity, int32_t P1, int32_t P2, int32_t uniqueness, int32_t flags,
                                 int32_t paths, const int16_t* d16_out) {
  return dense_stereo_check(fn, ctx, top, bot, n, rows, cols, min_disparity, P1, P2, uniqueness, flags, paths, d16_out);
}

int32_t sosvo_dense_launch_census(sosvo_ctx* ctx, const uint8_t* gray, int nimg, int rows, int cols, bool cyclic, uint64_t* out) {
  return launch_census(ctx, gray, nimg, rows, cols, cyclic, out);
}

int32_t sosvo_dense_stereo_run64(sosvo_ctx* ctx, const uint8_t* top, const uint8_t* bot, int32_t n, int32_t rows, int32_t cols,
                                 const uint8_t* mask, int32_t min_disparity, int32_t P1, int32_t P2, int32_t uniqueness, int32_t lr_max,
                                 int32_t flags, int32_t paths, int16_t* d16_out, uint16_t* S_out) {
  return dense_stereo_run(ctx, top, bot, n, rows, cols, mask, min_disparity, P1, P2, uniqueness, lr_max, flags, paths, d16_out, S_out);
}

extern "C" {

int32_t sosvo_census_9x7(sosvo_ctx* ctx, const uint8_t* gray, int32_t nimg, int32_t rows, int32_t cols, int32_t flags,
                         uint64_t* census_out) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, gray && census_out, "null pointer");
  SOSVO_REQUIRE_DENSE_SIZE(ctx, rows, cols);
  SOSVO_REQUIRE(ctx, nimg >= 1 && nimg <= 65535, "nimg out of range (1..65535)");
  SOSVO_REQUIRE_DENSE_FLAGS(ctx, flags);
  return launch_census(ctx, gray, nimg, rows, cols, (flags & SOSVO_DENSE_CYCLIC_COLUMNS) != 0, census_out);
}

int32_t sosvo_dense_stereo(sosvo_ctx* ctx, const uint8_t* top, const uint8_t* bot, int32_t n, int32_t rows, int32_t cols,
                           const uint8_t* mask, int32_t min_disparity, int32_t P1, int32_t P2, int32_t uniqueness,
                           int32_t lr_max, int32_t flags, int16_t* d16_out, uint16_t* S_out) {
  return dense_stereo_body(__func__, ctx, top, bot, n, rows, cols, mask, min_disparity, P1, P2, uniqueness, lr_max, flags, 4, d16_out, S_out);
}

int32_t sosvo_dense_stereo_paths(sosvo_ctx* ctx, const uint8_t* top, const uint8_t* bot, int32_t n, int32_t rows, int32_t cols,
                                 const uint8_t* mask, int32_t min_disparity, int32_t P1, int32_t P2, int32_t uniqueness,
                                 int32_t lr_max, int32_t flags, int32_t paths, int16_t* d16_out, uint16_t* S_out) {
  return dense_stereo_body(__func__, ctx, top, bot, n, rows, cols, mask, min_disparity, P1, P2, uniqueness, lr_max, flags, paths, d16_out,
                           S_out);
}

int32_t sosvo_dense_triangulate(sosvo_ctx* ctx, const sosvo_rig* rig_host, const int16_t* d16, int32_t n, int32_t rows,
                                int32_t cols, int32_t min_d16, int32_t max_d16, double* X_out) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, rig_host && d16 && X_out, "null pointer");
  SOSVO_REQUIRE_DENSE_SIZE(ctx, rows, cols);
  SOSVO_REQUIRE_DENSE_N(ctx, n);
  DenseRig rig;
  for (int k = 0; k < 4; ++k) {
    SOSVO_REQUIRE(ctx, rig_host->pano_top[k] == rig_host->pano_bot[k], "the rig's two panoramas differ in geometry");
    rig.pano_top[k] = rig_host->pano_top[k];
    rig.pano_bot[k] = rig_host->pano_bot[k];
  }
  for (int k = 0; k < 3; ++k) {
    rig.F_top[k] = rig_host->F_top[k];
    rig.F_bot[k] = rig_host->F_bot[k];
  }
  rig.min_range = rig_host->min_range;
  rig.max_range = rig_host->max_range;
  const size_t total = (size_t)n * rows * cols;
  SOSVO_LAUNCH(ctx, dense_triangulate_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, rig, d16, rows, cols, total,
               min_d16, max_d16, X_out);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

}  // extern "C"
