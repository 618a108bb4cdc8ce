// sosvo_refine_subpix -- cv2.cornerSubPix restated in exact integers: keypoints of the detectors,
// which sit on the pixel grid, move to the point whose offsets are orthogonal to the image gradients of a
// (2 half + 1)^2 window around it.  One wave per keypoint; the iteration is wave-uniform.
//
// Per iteration: the sampling centre is rounded to 1/32 px, the (2 half + 3)^2 bilinear samples around it are INTEGERS
// (weights (32 - f) and f on u8 pixels, at most 255 * 1024), central differences and the Gaussian weight table are
// integers too, and the five sums of the 2 x 2 normal equations are int64 (each below 2^55).  Exact integers: the sums do
// not depend on which lane adds what, and the CPU reference (tests/refsubpix.py) gets the same bits.  Only the 2 x 2
// solve is floating point -- FP64, every sum converted once, no contraction -- and is the same for every lane.
#include <math.h>

#include "common.h"

namespace {

constexpr int kMaxHalf = 5;
constexpr int kMaxSide = 2 * kMaxHalf + 3;  // samples per side: the window and one pixel around it for the differences

// w[k] = floor(256 exp(-((k - half) / half)^2) + 0.5), k = 0 .. 2 half: made on the host, once, by C's exp
struct SubpixWeights {
  int32_t w[2 * kMaxHalf + 1];
};
bool subpix_weights(int half, SubpixWeights& t) {
  if (half < 2 || half > kMaxHalf) return false;
  for (int k = 0; k < 2 * kMaxHalf + 1; ++k) t.w[k] = 0;
  for (int k = 0; k <= 2 * half; ++k) {
    const double r = (double)(k - half) / (double)half;
    t.w[k] = (int32_t)floor(256.0 * exp(-(r * r)) + 0.5);
  }
  return true;
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
  return v;
}

// Workgroup = one wave.  Workgroup (p, y) refines the keypoints y, y + gridDim.y, ... of problem p = image * nmask + mask.
// row_range: rows [first, last + 1) per view (image / imgs_per_range), nullptr = all rows; a range is cut to the image and
// to at least one row, so a sample never leaves the image.
__global__ __launch_bounds__(64) void subpix_refine_kernel(const uint8_t* __restrict__ gray, int rows, int cols, int nmask, int cap,
                                                           float* __restrict__ kp, const int32_t* __restrict__ n, int half,
                                                           int max_iter, double eps2, const int32_t* __restrict__ row_range,
                                                           int imgs_per_range, SubpixWeights wt) {
  __shared__ int32_t s_S[kMaxSide * kMaxSide];
  __shared__ int32_t s_w[2 * kMaxHalf + 1];
  const int lane = threadIdx.x;
  const int p = blockIdx.x, image = p / nmask;
  if (lane < 2 * kMaxHalf + 1) s_w[lane] = wt.w[lane];
  __syncthreads();
  const int count = min(__builtin_amdgcn_readfirstlane(n[p]), cap);
  int r0 = 0, r1 = rows;
  if (row_range) {
    const int v = image / imgs_per_range;
    r0 = clampi(row_range[2 * v], 0, rows - 1);
    r1 = clampi(row_range[2 * v + 1], r0 + 1, rows);
  }
  const uint8_t* img = gray + (size_t)image * rows * cols;
  const int side3 = 2 * half + 3, side1 = 2 * half + 1;
  const double hd = (double)half;

  for (int k = blockIdx.y; k < count; k += gridDim.y) {
    float* out = kp + ((size_t)p * cap + k) * 2;
    const float fx0 = out[0], fy0 = out[1];
    if (!(isfinite(fx0) && isfinite(fy0))) continue;  // (uniform: every lane read the same two floats)
    const double c0x = (double)fx0, c0y = (double)fy0;
    double cx = c0x, cy = c0y;
    for (int it = 0; it < max_iter; ++it) {
      // the centre on the 1/32-px grid: tq = 32 * base + frac, all exact in double whatever the magnitude
      const double tqx = floor(32.0 * cx + 0.5), tqy = floor(32.0 * cy + 0.5);
      const double bx = floor(tqx * 0.03125), by = floor(tqy * 0.03125);
      const int fx = (int)(tqx - 32.0 * bx), fy = (int)(tqy - 32.0 * by);
      // (a base far outside the image clamps like one 32 px outside: the offsets are at most half + 2 <= 7)
      const int ix = (int)fmin(fmax(bx, -32.0), (double)cols + 32.0), iy = (int)fmin(fmax(by, -32.0), (double)rows + 32.0);
      for (int s = lane; s < side3 * side3; s += 64) {
        const int i = s / side3, j = s - i * side3;
        const int x = ix + j - half - 1, y = iy + i - half - 1;
        const int x0 = clampi(x, 0, cols - 1), x1 = clampi(x + 1, 0, cols - 1);
        const int y0 = clampi(y, r0, r1 - 1), y1 = clampi(y + 1, r0, r1 - 1);
        const int p00 = img[(size_t)y0 * cols + x0], p01 = img[(size_t)y0 * cols + x1];
        const int p10 = img[(size_t)y1 * cols + x0], p11 = img[(size_t)y1 * cols + x1];
        s_S[s] = (32 - fy) * ((32 - fx) * p00 + fx * p01) + fy * ((32 - fx) * p10 + fx * p11);
      }
      __syncthreads();
      long long a = 0, b = 0, c2 = 0, b1 = 0, b2 = 0;
      for (int e = lane; e < side1 * side1; e += 64) {
        const int i = e / side1, j = e - i * side1;
        const long long gx = s_S[(i + 1) * side3 + j + 2] - s_S[(i + 1) * side3 + j];
        const long long gy = s_S[(i + 2) * side3 + j + 1] - s_S[i * side3 + j + 1];
        const long long m = (s_w[i] * s_w[j]) >> 8;
        const long long gxx = gx * gx * m, gxy = gx * gy * m, gyy = gy * gy * m;
        const long long px = j - half, py = i - half;
        a += gxx;
        b += gxy;
        c2 += gyy;
        b1 += gxx * px + gxy * py;
        b2 += gxy * px + gyy * py;
      }
      __syncthreads();  // (the next iteration writes s_S)
      const double A = (double)wave_sum(a), B = (double)wave_sum(b), C = (double)wave_sum(c2);
      const double B1 = (double)wave_sum(b1), B2 = (double)wave_sum(b2);
      const double det = A * C - B * B;
      if (det == 0.0) break;
      const double nx = tqx * 0.03125 + (C * B1 - B * B2) / det, ny = tqy * 0.03125 + (A * B2 - B * B1) / det;
      const double dx = nx - cx, dy = ny - cy;
      const double err = dx * dx + dy * dy;
      if (!(fabs(nx - c0x) <= hd && fabs(ny - c0y) <= hd)) {  // left the window of the start (or NaN): the start stands
        cx = c0x;
        cy = c0y;
        break;
      }
      cx = nx;
      cy = ny;
      if (err <= eps2) break;
    }
    if (lane == 0) {
      out[0] = (float)cx;
      out[1] = (float)cy;
    }
  }
}

}  // namespace

extern "C" {

int32_t sosvo_subpix_weights(sosvo_ctx* ctx, int32_t half, int32_t* w_host) {
  SubpixWeights t;
  if (!w_host) return sosvo_fail(ctx, SOSVO_ERR_ARG, __func__, "null pointer");
  if (!subpix_weights(half, t)) return sosvo_fail(ctx, SOSVO_ERR_ARG, __func__, "half out of range (2..5)");
  for (int k = 0; k <= 2 * half; ++k) w_host[k] = t.w[k];
  return SOSVO_OK;
}

int32_t sosvo_refine_subpix(sosvo_ctx* ctx, const uint8_t* gray, int32_t nimg, int32_t rows, int32_t cols, int32_t nmask,
                            int32_t cap, float* kp, const int32_t* n, int32_t half, int32_t max_iter, double eps,
                            const int32_t* row_range) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, gray && kp && n, "null pointer");
  SOSVO_REQUIRE(ctx, row_range == nullptr || nimg % 2 == 0, "row_range needs the two views' images (nimg even, view-major)");
  SOSVO_REQUIRE(ctx, nimg >= 0 && nimg <= 65535 && nmask >= 1 && nimg * (int64_t)nmask < (1 << 24), "nimg / nmask out of range");
  SOSVO_REQUIRE(ctx, rows >= 1 && cols >= 1 && rows * (int64_t)cols < (1 << 28), "image sizes out of range");
  SOSVO_REQUIRE(ctx, cap > 0 && cap <= 4096, "cap out of range");
  SubpixWeights wt;
  SOSVO_REQUIRE(ctx, subpix_weights(half, wt), "half out of range (2..5)");
  SOSVO_REQUIRE(ctx, max_iter >= 1, "max_iter must be at least 1");
  SOSVO_REQUIRE(ctx, eps >= 0.0, "eps must not be negative or NaN");
  if (nimg == 0) return SOSVO_OK;
  // waves per problem: enough for the chip at a few problems, a few keypoints per wave at thousands
  const int P = nimg * nmask, per = P >= 4096 ? 16 : 64;
  SOSVO_LAUNCH(ctx, subpix_refine_kernel, dim3(P, min(cap, per)), dim3(64), 0, ctx->stream, gray, rows, cols, nmask, cap, kp, n,
               half, max_iter, eps * eps, row_range, nimg > 1 ? nimg / 2 : 1, wt);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

}  // extern "C"
