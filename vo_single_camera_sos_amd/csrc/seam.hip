// The seam-free front end (SOSVO_FLAG_SEAM_FREE): the plain front end run on panoramas padded by
// SOSVO_SEAM_HALO columns of their own cyclic neighbours on either side.  The tuned image kernels are not touched; they run
// at cols + 2 * SOSVO_SEAM_HALO columns.  Here are the small stages around them: the mask bits with an empty halo (every
// original pixel is detected exactly once), the keypoints back to the period's columns, the interior of a padded gray batch.
// (The padded unwrap table is sosvo_unwrap_prepare_seam_free in image.hip, the store's padded level-0 fill in lk.hip.)
#include "common.h"

namespace {

constexpr int kHalo = SOSVO_SEAM_HALO;

// out[set, r, c'] = bits[set, r, c' - HALO] inside [HALO, HALO + cols), 0 in the halo
__global__ __launch_bounds__(256) void seam_mask_bits_kernel(const uint32_t* __restrict__ bits, int cols, uint32_t* __restrict__ out) {
  const int cp = blockIdx.x * 256 + threadIdx.x, colsp = cols + 2 * kHalo;
  if (cp >= colsp) return;
  const size_t row = blockIdx.y + (size_t)blockIdx.z * gridDim.y;  // set * rows + r
  const int c = cp - kHalo;
  out[row * colsp + cp] = c >= 0 && c < cols ? bits[row * cols + c] : 0u;
}

// x = x' - HALO, + period if negative, - period if >= period, and `period` itself is column 0 (float32 throughout)
__global__ __launch_bounds__(256) void seam_keypoints_unpad_kernel(float* __restrict__ kp, const int32_t* __restrict__ n, int nprob,
                                                                   int cap, float period) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  for (int p = blockIdx.y; p < nprob; p += gridDim.y) {
    if (i >= min(n[p], cap)) continue;
    float* px = kp + ((size_t)p * cap + i) * 2;
    float x = *px - (float)kHalo;
    if (x < 0.0f) x += period;
    if (x >= period) x -= period;
    if (x == period) x = 0.0f;
    *px = x;
  }
}

// the rows [r0, r1) of the view's range of image blockIdx.y: the columns [HALO, HALO + cols) of gray -> out
__global__ __launch_bounds__(256) void seam_gray_unpad_kernel(const uint8_t* __restrict__ gray, int imgs_per_view, int rows, int cols,
                                                              const int32_t* __restrict__ row_range, uint8_t* __restrict__ out) {
  const int img = blockIdx.y, v = img / imgs_per_view;
  int r0 = 0, r1 = rows;
  if (row_range) {
    r0 = max(0, min(rows, row_range[2 * v]));
    r1 = max(r0, min(rows, row_range[2 * v + 1]));
  }
  const size_t pitch = (size_t)cols + 2 * kHalo;
  sosvo_copy_rows(out + ((size_t)img * rows + r0) * cols, (size_t)cols, gray + ((size_t)img * rows + r0) * pitch + kHalo, pitch, cols,
                  r1 - r0, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

}  // namespace

extern "C" {

int32_t sosvo_mask_bits_seam_free(sosvo_ctx* ctx, const uint32_t* mask_bits, int32_t nsets, int32_t rows, int32_t cols,
                                  uint32_t* out) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, mask_bits && out, "null pointer");
  SOSVO_REQUIRE(ctx, nsets >= 1 && nsets <= 65535, "nsets out of range");
  SOSVO_REQUIRE(ctx, rows > 0 && rows <= 65535 && cols > 0 && rows * ((int64_t)cols + 2 * kHalo) < (1 << 28), "image sizes out of range");
  SOSVO_LAUNCH(ctx, seam_mask_bits_kernel, dim3(cdiv(cols + 2 * kHalo, 256), rows, nsets), dim3(256), 0, ctx->stream, mask_bits, cols,
               out);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

int32_t sosvo_keypoints_unpad(sosvo_ctx* ctx, float* kp, const int32_t* n, int32_t nprob, int32_t cap, int32_t period) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, kp && n, "null pointer");
  SOSVO_REQUIRE(ctx, nprob >= 0 && nprob <= (1 << 24) && cap > 0 && cap <= (1 << 24), "nprob / cap out of range");
  SOSVO_REQUIRE(ctx, period >= 1 && period <= 16384, "period out of range (1..16384)");
  if (nprob == 0) return SOSVO_OK;
  SOSVO_LAUNCH(ctx, seam_keypoints_unpad_kernel, dim3(cdiv(cap, 256), min(nprob, 65535)), dim3(256), 0, ctx->stream, kp, n,
               nprob, cap, (float)period);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

int32_t sosvo_gray_unpad(sosvo_ctx* ctx, const uint8_t* gray, int32_t nimg, int32_t rows, int32_t cols, const int32_t* row_range,
                         uint8_t* out) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, gray && out, "null pointer");
  SOSVO_REQUIRE(ctx, nimg >= 0 && nimg <= 65535, "nimg out of range");
  SOSVO_REQUIRE(ctx, rows >= 1 && cols >= 1 && rows * ((int64_t)cols + 2 * kHalo) < (1 << 28), "image sizes out of range");
  SOSVO_REQUIRE(ctx, row_range == nullptr || nimg % 2 == 0, "row_range needs the two views' images (nimg even, view-major)");
  if (nimg == 0) return SOSVO_OK;
  const int blocks = min(cdiv(rows * cols, 4096), 64);
  SOSVO_LAUNCH(ctx, seam_gray_unpad_kernel, dim3(blocks, nimg), dim3(256), 0, ctx->stream, gray, nimg > 1 ? nimg / 2 : 1, rows, cols,
               row_range, out);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

}  // extern "C"
