// WLS filter of the dense disparity map: the confidence of include/sosvo_dense_filter.h and the
// fast global smoother over the confidence-weighted map (tests/refwls.py is the same text in numpy).  Every double
// operation below is written once, in the header's order, and -ffp-contract=off keeps it one rounding each: the planes and
// the map equal the numpy statement bit for bit.
//
// The right-hand sides N and D live in scratch as planes [n, rows, cols].  One iteration is four launches:
//   rows forward / rows backward: one lane per (frame, row), 64 rows per single-wave workgroup.  A lane walking its row in
//     global memory would read with a stride of cols, so a tile of 64 rows by 16 columns goes through LDS: loaded with whole
//     128-byte row segments, walked by every lane along its own row, and written back the same way; the next tile's loads are
//     in flight during the walk.  The cyclic form carries a third right-hand side, and a fifth launch, one lane per pixel,
//     applies the Sherman-Morrison correction.
//   cols forward / cols backward: one lane per (frame, column), consecutive lanes on consecutive columns, so every step's
//     loads and stores are whole lines already.
// Each step has one FP64 reciprocal in its dependency chain; the kernels are latency-bound by construction.
#include "common.h"
#include "dense_wls_scratch.h"
#include "sosvo_dense_filter.h"

namespace {

constexpr int kTileRows = 64;              // one wave: a lane per row
constexpr int kTileCols = 16;              // 128 bytes of a double plane per row and tile
constexpr int kPitch = kTileCols + 1;      // (odd: the lanes of a walk spread over the banks)
constexpr int kPieces = kTileRows / 4;     // a wave instruction moves 4 rows of 16 columns: lane -> (lane / 16 + 4 k, lane % 16)

struct wls_table {
  double w[SOSVO_WLS_WEIGHTS];
};

__global__ __launch_bounds__(256) void wls_confidence_kernel(const int16_t* __restrict__ d16, int rows, int cols, int radius,
                                                             int roll_ppm, int cyclic, uint8_t* __restrict__ conf) {
  const uint32_t frame_pixels = (uint32_t)rows * cols, p = blockIdx.x * 256u + threadIdx.x;
  if (p >= frame_pixels) return;
  const size_t f0 = (size_t)blockIdx.y * frame_pixels;
  const int16_t* d = d16 + f0;
  if (d[p] < 0) {
    conf[f0 + p] = 0;
    return;
  }
  const int r = (int)(p / (uint32_t)cols), c = (int)(p - (uint32_t)r * cols);
  int32_t m = 0, s1 = 0;  // (s1 <= 225 * 32767)
  int64_t s2 = 0;
  for (int dy = -radius; dy <= radius; ++dy) {
    const int rr = r + dy;
    if (rr < 0 || rr >= rows) continue;
    for (int dx = -radius; dx <= radius; ++dx) {
      int cc = c + dx;
      if (cyclic) {
        cc %= cols;
        if (cc < 0) cc += cols;
      } else if (cc < 0 || cc >= cols) {
        continue;
      }
      const int32_t t = d[(uint32_t)rr * cols + cc];
      if (t >= 0) {
        m += 1;
        s1 += t;
        s2 += t * t;
      }
    }
  }
  const int64_t V = ((int64_t)m * s2 - (int64_t)s1 * s1) / ((int64_t)m * m);  // (the numerator is not negative: floor = truncation)
  const int64_t v = 255 - (255 * (int64_t)roll_ppm * V) / 1000000;
  conf[f0 + p] = (uint8_t)(v < 0 ? 0 : v);
}

// Step 1: the two right-hand sides; the only reader of d16 and conf.  Workgroup (0, 0) also puts the caller's table, which
// travels in the kernel's arguments, into scratch.
__global__ __launch_bounds__(256) void wls_init_kernel(const int16_t* __restrict__ d16, const uint8_t* __restrict__ conf, int rows, int cols,
                                                       wls_table table, double* __restrict__ N, double* __restrict__ D,
                                                       double* __restrict__ weights) {
  if (blockIdx.x == 0 && blockIdx.y == 0) weights[threadIdx.x] = table.w[threadIdx.x];
  const uint32_t frame_pixels = (uint32_t)rows * cols, p = blockIdx.x * 256u + threadIdx.x;
  if (p >= frame_pixels) return;
  const size_t i = (size_t)blockIdx.y * frame_pixels + p;
  const int32_t d = d16[i];
  const int32_t w = d >= 0 ? (conf ? (int32_t)conf[i] : 255) : 0;
  N[i] = (double)(w * d);
  D[i] = (double)w;
}

// lam_t * weights[k] for the workgroup (64 threads)
__device__ __forceinline__ void scaled_table(double* wt, const double* __restrict__ weights, double lam) {
  for (int k = threadIdx.x; k < SOSVO_WLS_WEIGHTS; k += 64) wt[k] = lam * weights[k];
  __syncthreads();
}

// ---- along the columns of the map: one lane per (frame, column) -------------------------------------------------------------
__global__ __launch_bounds__(64) void wls_cols_forward_kernel(const uint8_t* __restrict__ guide, const double* __restrict__ weights, double lam,
                                                              size_t lines, int rows, int cols, const double* __restrict__ N,
                                                              const double* __restrict__ D, double* __restrict__ cp,
                                                              double* __restrict__ fN, double* __restrict__ fD) {
  __shared__ double wt[SOSVO_WLS_WEIGHTS];
  scaled_table(wt, weights, lam);
  const size_t line = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (line >= lines) return;
  const size_t frame = line / (size_t)cols;
  size_t p = frame * rows * cols + (line - frame * cols);
  int g = guide[p];
  double wl = 0.0, cpp = 0.0, pN = 0.0, pD = 0.0;
  for (int i = 0; i < rows; ++i, p += cols) {
    const bool first = i == 0, last = i == rows - 1;
    const int gn = last ? g : (int)guide[p + cols];
    const double wr = last ? 0.0 : wt[abs(gn - g)];
    const double b = (1.0 + wl) + wr, a = -wl, c = -wr;
    const double r = 1.0 / (first ? b : b - a * cpp);
    cpp = c * r;
    const double n_i = N[p], d_i = D[p];
    pN = (first ? n_i : n_i - a * pN) * r;
    pD = (first ? d_i : d_i - a * pD) * r;
    cp[p] = cpp;
    fN[p] = pN;
    fD[p] = pD;
    wl = wr;
    g = gn;
  }
}

__global__ __launch_bounds__(64) void wls_cols_backward_kernel(size_t lines, int rows, int cols, const double* __restrict__ cp,
                                                               const double* __restrict__ fN, const double* __restrict__ fD,
                                                               double* __restrict__ N, double* __restrict__ D) {
  const size_t line = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (line >= lines) return;
  const size_t frame = line / (size_t)cols;
  size_t p = frame * rows * cols + (line - frame * cols) + (size_t)(rows - 1) * cols;
  double uN = fN[p], uD = fD[p];
  N[p] = uN;
  D[p] = uD;
  for (int i = rows - 2; i >= 0; --i) {
    p -= cols;
    const double c = cp[p];
    uN = fN[p] - c * uN;
    uD = fD[p] - c * uD;
    N[p] = uN;
    D[p] = uD;
  }
}

// ---- along the rows of the map: one lane per (frame, row), tiles through LDS -------------------------------------------------
// The rows of all frames are the rows of one matrix [lines, cols], lines = n * rows.

// Tile element (row, col) of this lane's k-th piece: 4 rows of 16 columns per wave instruction.
#define WLS_TILE_PIECES(row, col)                                  \
  for (int k_ = 0, row = threadIdx.x >> 4, col = threadIdx.x & 15; k_ < kTileRows / 4; ++k_, row += 4)

template <bool CYC>
__global__ __launch_bounds__(64) void wls_rows_forward_kernel(const uint8_t* __restrict__ guide, const double* __restrict__ weights, double lam,
                                                              size_t lines, int cols, const double* __restrict__ N,
                                                              const double* __restrict__ D, double* __restrict__ cp,
                                                              double* __restrict__ fN, double* __restrict__ fD, double* __restrict__ fz) {
  __shared__ double wt[SOSVO_WLS_WEIGHTS];
  __shared__ double tN[kTileRows][kPitch], tD[kTileRows][kPitch], tC[kTileRows][kPitch], tZ[CYC ? kTileRows : 1][kPitch];
  __shared__ uint8_t tg[kTileRows][kTileCols];
  scaled_table(wt, weights, lam);
  const int lane = threadIdx.x, prow = lane >> 4, pcol = lane & 15;
  const size_t line0 = (size_t)blockIdx.x * kTileRows;
  const bool active = line0 + lane < lines;
  const size_t own = (line0 + lane) * (size_t)cols;
  double wl = 0.0, cpp = 0.0, pN = 0.0, pD = 0.0, pZ = 0.0, ws = 0.0, nws = 0.0, gamma = 0.0;
  if (CYC && active) {
    ws = wt[abs((int)guide[own] - (int)guide[own + cols - 1])];
    nws = -ws;
  }
  // The next tile travels in registers while this one is walked: its loads are issued before the walk and land in LDS after
  // it, so the walk hides their latency (a single wave has nothing else to hide it with).
  double rN[kPieces], rD[kPieces];
  int rg[kPieces], g_after = 0;  // g_after: the lane's own guide value one column past the tile
  auto fetch = [&](int c0) {
    const int tc = min(kTileCols, cols - c0);
#pragma unroll
    for (int k = 0; k < kPieces; ++k) {
      const int row = prow + 4 * k;
      const bool in = line0 + row < lines && pcol < tc;
      const size_t i = (line0 + row) * (size_t)cols + c0 + pcol;
      rN[k] = in ? N[i] : 0.0;
      rD[k] = in ? D[i] : 0.0;
      rg[k] = in ? (int)guide[i] : 0;
    }
    g_after = (active && c0 + kTileCols < cols) ? (int)guide[own + c0 + kTileCols] : 0;
  };
  fetch(0);
  for (int c0 = 0; c0 < cols; c0 += kTileCols) {
    const int tc = min(kTileCols, cols - c0);
    __syncthreads();  // (the previous tile's stores have read the LDS)
#pragma unroll
    for (int k = 0; k < kPieces; ++k) {
      tN[prow + 4 * k][pcol] = rN[k];
      tD[prow + 4 * k][pcol] = rD[k];
      tg[prow + 4 * k][pcol] = (uint8_t)rg[k];
    }
    const int g_end = g_after;
    __syncthreads();
    if (c0 + kTileCols < cols) fetch(c0 + kTileCols);
    if (active) {
      // what does not depend on the previous step first, for all 16 columns (past the row's end: zeros, unused) ...
      double wrj[kTileCols], nj[kTileCols], dj[kTileCols];
#pragma unroll
      for (int j = 0; j < kTileCols; ++j) {
        const int g = tg[lane][j], gn = j + 1 < kTileCols ? (int)tg[lane][j + 1] : g_end;
        wrj[j] = c0 + j >= cols - 1 ? 0.0 : wt[abs(gn - g)];
        nj[j] = tN[lane][j];
        dj[j] = tD[lane][j];
      }
      // ... then the chain
#pragma unroll
      for (int j = 0; j < kTileCols; ++j) {
        if (j < tc) {
          const bool first = c0 + j == 0, last = c0 + j == cols - 1;
          const double wr = wrj[j];
          double b;
          if (CYC && first) {
            const double b0 = (1.0 + ws) + wr;
            gamma = -b0;
            b = b0 - gamma;
          } else if (CYC && last) {
            b = (1.0 + wl) + ws;
            b = b - (nws * nws) / gamma;
          } else {
            b = (1.0 + wl) + wr;
          }
          const double a = -wl, c = -wr;
          const double r = 1.0 / (first ? b : b - a * cpp);
          cpp = c * r;
          pN = (first ? nj[j] : nj[j] - a * pN) * r;
          pD = (first ? dj[j] : dj[j] - a * pD) * r;
          tC[lane][j] = cpp;
          tN[lane][j] = pN;
          tD[lane][j] = pD;
          if (CYC) {
            const double z_i = first ? gamma : (last ? nws : 0.0);
            pZ = (first ? z_i : z_i - a * pZ) * r;
            tZ[lane][j] = pZ;
          }
          wl = wr;
        }
      }
    }
    __syncthreads();
    WLS_TILE_PIECES(row, col) {
      if (line0 + row < lines && col < tc) {
        const size_t i = (line0 + row) * (size_t)cols + c0 + col;
        cp[i] = tC[row][col];
        fN[i] = tN[row][col];
        fD[i] = tD[row][col];
        if (CYC) fz[i] = tZ[row][col];
      }
    }
  }
}

// With CYC the plane fz is read (f') and written (z) tile by tile: no __restrict__ on it.
template <bool CYC>
__global__ __launch_bounds__(64) void wls_rows_backward_kernel(const uint8_t* __restrict__ guide, const double* __restrict__ weights, double lam,
                                                               size_t lines, int cols, const double* __restrict__ cp,
                                                               const double* __restrict__ fN, const double* __restrict__ fD, double* fz,
                                                               double* __restrict__ N, double* __restrict__ D, double* __restrict__ ratio) {
  __shared__ double wt[CYC ? SOSVO_WLS_WEIGHTS : 1];
  __shared__ double tN[kTileRows][kPitch], tD[kTileRows][kPitch], tC[kTileRows][kPitch], tZ[CYC ? kTileRows : 1][kPitch];
  if (CYC) scaled_table(wt, weights, lam);
  const int lane = threadIdx.x, prow = lane >> 4, pcol = lane & 15;
  const size_t line0 = (size_t)blockIdx.x * kTileRows;
  const bool active = line0 + lane < lines;
  double uN = 0.0, uD = 0.0, uZ = 0.0, lastN = 0.0, lastD = 0.0, lastZ = 0.0;
  double rC[kPieces], rN[kPieces], rD[kPieces], rZ[CYC ? kPieces : 1];  // the next tile, as in the forward kernel
  auto fetch = [&](int c0) {
    const int tc = min(kTileCols, cols - c0);
#pragma unroll
    for (int k = 0; k < kPieces; ++k) {
      const int row = prow + 4 * k;
      const bool in = line0 + row < lines && pcol < tc;
      const size_t i = (line0 + row) * (size_t)cols + c0 + pcol;
      rC[k] = in ? cp[i] : 0.0;
      rN[k] = in ? fN[i] : 0.0;
      rD[k] = in ? fD[i] : 0.0;
      if (CYC) rZ[k] = in ? fz[i] : 0.0;
    }
  };
  const int c_last = ((cols - 1) / kTileCols) * kTileCols;
  fetch(c_last);
  for (int c0 = c_last; c0 >= 0; c0 -= kTileCols) {
    const int tc = min(kTileCols, cols - c0);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPieces; ++k) {
      tC[prow + 4 * k][pcol] = rC[k];
      tN[prow + 4 * k][pcol] = rN[k];
      tD[prow + 4 * k][pcol] = rD[k];
      if (CYC) tZ[prow + 4 * k][pcol] = rZ[k];
    }
    __syncthreads();
    if (c0 > 0) fetch(c0 - kTileCols);
    if (active) {
      double cj[kTileCols], nj[kTileCols], dj[kTileCols], zj[CYC ? kTileCols : 1];
#pragma unroll
      for (int j = 0; j < kTileCols; ++j) {
        cj[j] = tC[lane][j];
        nj[j] = tN[lane][j];
        dj[j] = tD[lane][j];
        if (CYC) zj[j] = tZ[lane][j];
      }
#pragma unroll
      for (int j = kTileCols - 1; j >= 0; --j) {
        if (j < tc) {
          const bool last = c0 + j == cols - 1;
          uN = last ? nj[j] : nj[j] - cj[j] * uN;
          uD = last ? dj[j] : dj[j] - cj[j] * uD;
          tN[lane][j] = uN;
          tD[lane][j] = uD;
          if (CYC) {
            uZ = last ? zj[j] : zj[j] - cj[j] * uZ;
            tZ[lane][j] = uZ;
            if (last) lastN = uN, lastD = uD, lastZ = uZ;
          }
        }
      }
    }
    __syncthreads();
    WLS_TILE_PIECES(row, col) {
      if (line0 + row < lines && col < tc) {
        const size_t i = (line0 + row) * (size_t)cols + c0 + col;
        N[i] = tN[row][col];
        D[i] = tD[row][col];
        if (CYC) fz[i] = tZ[row][col];
      }
    }
  }
  if (!CYC) return;
  // Sherman-Morrison: the row's vy / vz for wls_rows_correct_kernel, the lane's uN, uD, uZ being y_0, z_0 now
  if (active) {
    const size_t own = (line0 + lane) * (size_t)cols;
    const int g0 = guide[own], g1 = guide[own + 1], gl = guide[own + cols - 1];
    const double ws = wt[abs(g0 - gl)], wr0 = wt[abs(g1 - g0)];
    const double b0 = (1.0 + ws) + wr0, gamma = -b0, q = (-ws) / gamma;
    const double vz = 1.0 + (uZ + q * lastZ);
    const double vyN = uN + q * lastN, vyD = uD + q * lastD;
    ratio[2 * (line0 + lane)] = vyN / vz;
    ratio[2 * (line0 + lane) + 1] = vyD / vz;
  }
}

// ... and x = y - z (vy / vz) itself, one lane per pixel: inside the backward kernel this pass had one wave per 64 rows to
// move three planes with, and took longer than the sweep.
__global__ __launch_bounds__(256) void wls_rows_correct_kernel(const double* __restrict__ z, const double* __restrict__ ratio, int rows,
                                                               int cols, double* __restrict__ N, double* __restrict__ D) {
  const uint32_t frame_pixels = (uint32_t)rows * cols, p = blockIdx.x * 256u + threadIdx.x;
  if (p >= frame_pixels) return;
  const size_t i = (size_t)blockIdx.y * frame_pixels + p, line = (size_t)blockIdx.y * rows + p / (uint32_t)cols;
  const double z_i = z[i];
  N[i] = N[i] - z_i * ratio[2 * line];
  D[i] = D[i] - z_i * ratio[2 * line + 1];
}

// Step 5
__global__ __launch_bounds__(256) void wls_final_kernel(const double* __restrict__ N, const double* __restrict__ D,
                                                        const uint8_t* __restrict__ mask, int rows, int cols, double min_den,
                                                        int16_t* __restrict__ d16_out, double* __restrict__ planes_out) {
  const uint32_t frame_pixels = (uint32_t)rows * cols, p = blockIdx.x * 256u + threadIdx.x;
  if (p >= frame_pixels) return;
  const size_t i = (size_t)blockIdx.y * frame_pixels + p;
  const double num = N[i], den = D[i];
  int16_t out = -1;
  if (den >= min_den && (!mask || mask[p] != 0)) {
    double v = floor(num / den + 0.5);
    v = v < 0.0 ? 0.0 : (v > 32767.0 ? 32767.0 : v);
    out = (int16_t)v;
  }
  d16_out[i] = out;
  if (planes_out) {
    planes_out[2 * (size_t)blockIdx.y * frame_pixels + p] = num;
    planes_out[(2 * (size_t)blockIdx.y + 1) * frame_pixels + p] = den;
  }
}

}  // namespace

extern "C" int32_t sosvo_dense_confidence(sosvo_ctx* ctx, const int16_t* d16, int32_t n, int32_t rows, int32_t cols, int32_t radius,
                                          int32_t roll_ppm, int32_t flags, uint8_t* conf_out) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, d16 && conf_out, "null pointer");
  SOSVO_REQUIRE_DENSE_SIZE(ctx, rows, cols);
  SOSVO_REQUIRE_DENSE_N(ctx, n);
  SOSVO_REQUIRE(ctx, radius >= 0 && radius <= SOSVO_WLS_MAX_RADIUS, "radius out of range (0..7)");
  SOSVO_REQUIRE(ctx, roll_ppm >= 0 && roll_ppm <= SOSVO_WLS_MAX_ROLL_PPM, "roll_ppm out of range (0..1000000)");
  SOSVO_REQUIRE_DENSE_FLAGS(ctx, flags);
  const size_t frame_pixels = (size_t)rows * cols;
  SOSVO_LAUNCH(ctx, wls_confidence_kernel, dim3((unsigned)((frame_pixels + 255) / 256), n), dim3(256), 0, ctx->stream, d16, rows, cols,
               radius, roll_ppm, (flags & SOSVO_DENSE_CYCLIC_COLUMNS) != 0 ? 1 : 0, conf_out);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

extern "C" int32_t sosvo_dense_wls(sosvo_ctx* ctx, const int16_t* d16, const uint8_t* guide, const uint8_t* conf, const uint8_t* mask,
                                   int32_t n, int32_t rows, int32_t cols, double lambda, const double* weights, int32_t iters,
                                   double min_weight, int32_t flags, int16_t* d16_out, double* planes_out) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, d16 && guide && weights && d16_out, "null pointer");
  SOSVO_REQUIRE_DENSE_SIZE(ctx, rows, cols);
  SOSVO_REQUIRE_DENSE_N(ctx, n);
  SOSVO_REQUIRE(ctx, lambda >= 0.0 && lambda <= SOSVO_WLS_MAX_LAMBDA, "lambda out of range (0..1e6)");
  wls_table table;
  for (int k = 0; k < SOSVO_WLS_WEIGHTS; ++k) {
    SOSVO_REQUIRE(ctx, weights[k] >= 0.0 && weights[k] <= 1.0, "weights: an entry is not a finite number in 0..1");
    table.w[k] = weights[k];
  }
  SOSVO_REQUIRE(ctx, iters >= 1 && iters <= SOSVO_WLS_MAX_ITERS, "iters out of range (1..8)");
  SOSVO_REQUIRE(ctx, min_weight > 0.0 && min_weight <= 1.7976931348623157e308, "min_weight is not a finite positive number");
  SOSVO_REQUIRE_DENSE_FLAGS(ctx, flags);
  const size_t frame_pixels = (size_t)rows * cols, total = (size_t)n * frame_pixels;
  const bool cyclic_rows = (flags & SOSVO_DENSE_CYCLIC_COLUMNS) != 0 && cols >= 3;
  sosvo_dense_wls_scratch s;
  const int32_t rc = sosvo_ws_carve(ctx, [&](Carver& cv) { s = sosvo_dense_wls_carve(cv, total, (size_t)n * rows, cyclic_rows); });
  if (rc != SOSVO_OK) return rc;
  const dim3 per_pixel((unsigned)((frame_pixels + 255) / 256), n);
  const size_t row_lines = (size_t)n * rows, col_lines = (size_t)n * cols;
  const dim3 row_grid((unsigned)((row_lines + kTileRows - 1) / kTileRows)), col_grid((unsigned)((col_lines + 63) / 64));
  SOSVO_LAUNCH(ctx, wls_init_kernel, per_pixel, dim3(256), 0, ctx->stream, d16, conf, rows, cols, table, s.N, s.D, s.weights);
  SOSVO_LAUNCH_CHECK(ctx);
  for (int t = 0; t < iters; ++t) {
    const double lam = ((1.5 * lambda) * (double)(1 << (2 * (iters - 1 - t)))) / (double)((1 << (2 * iters)) - 1);
    if (cyclic_rows) {
      SOSVO_LAUNCH_AS(ctx, "wls_rows_forward_kernel", wls_rows_forward_kernel<true>, row_grid, dim3(64), 0, ctx->stream, guide, s.weights,
                      lam, row_lines, cols, s.N, s.D, s.cp, s.fN, s.fD, s.fz);
      SOSVO_LAUNCH_CHECK(ctx);
      SOSVO_LAUNCH_AS(ctx, "wls_rows_backward_kernel", wls_rows_backward_kernel<true>, row_grid, dim3(64), 0, ctx->stream, guide, s.weights,
                      lam, row_lines, cols, s.cp, s.fN, s.fD, s.fz, s.N, s.D, s.ratio);
      SOSVO_LAUNCH_CHECK(ctx);
      SOSVO_LAUNCH(ctx, wls_rows_correct_kernel, per_pixel, dim3(256), 0, ctx->stream, s.fz, s.ratio, rows, cols, s.N, s.D);
    } else {
      SOSVO_LAUNCH_AS(ctx, "wls_rows_forward_kernel", wls_rows_forward_kernel<false>, row_grid, dim3(64), 0, ctx->stream, guide, s.weights,
                      lam, row_lines, cols, s.N, s.D, s.cp, s.fN, s.fD, s.fz);
      SOSVO_LAUNCH_CHECK(ctx);
      SOSVO_LAUNCH_AS(ctx, "wls_rows_backward_kernel", wls_rows_backward_kernel<false>, row_grid, dim3(64), 0, ctx->stream, guide, s.weights,
                      lam, row_lines, cols, s.cp, s.fN, s.fD, s.fz, s.N, s.D, s.ratio);
    }
    SOSVO_LAUNCH_CHECK(ctx);
    SOSVO_LAUNCH(ctx, wls_cols_forward_kernel, col_grid, dim3(64), 0, ctx->stream, guide, s.weights, lam, col_lines, rows, cols, s.N, s.D,
                 s.cp, s.fN, s.fD);
    SOSVO_LAUNCH_CHECK(ctx);
    SOSVO_LAUNCH(ctx, wls_cols_backward_kernel, col_grid, dim3(64), 0, ctx->stream, col_lines, rows, cols, s.cp, s.fN, s.fD, s.N, s.D);
    SOSVO_LAUNCH_CHECK(ctx);
  }
  SOSVO_LAUNCH(ctx, wls_final_kernel, per_pixel, dim3(256), 0, ctx->stream, s.N, s.D, mask, rows, cols, 255.0 * min_weight, d16_out,
               planes_out);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}
