// Dense omnistereo with D = 16 .. 256 disparities (include/sosvo_dense_wide.h; tests/refdense_wide.py is
// the same text in numpy): the algorithm of dense.hip with 64 replaced by D in the volumes' last axis, the recurrence's two
// ends, the winner and the parabola's two ends.  The reference tuner's num_of_disparities (common_cv.py:491).
//
// The wave stays one pixel of one scan line.  A lane owns W consecutive disparities, k = lane * W + j, W = 1 / 2 / 4 for
// D <= 64 / 128 / 256 (a template parameter).  D is a multiple of 16 and W divides 16, so a lane is either wholly inside the
// volume or wholly outside: the lanes at k >= D carry kBig in L, load and store nothing, and lose every minimum.  A lane's W
// bytes of C and 2 W bytes of S are one aligned load each (u8 / u16 / u32 and u16 / u32 / u64), so a wave reads and writes
// the whole contiguous line of D and 2 D bytes of its pixel.  The k - 1 / k + 1 terms are register neighbours; only slot 0
// and slot W - 1 take the whole-wave shifts of common.h.  The path minimum is W - 1 min in the lane and one wave_min.
// With 64 disparities the entry point runs dense.hip's body: these kernels run for every other D.
#include "common.h"
#include "dense_wide_scratch.h"
#include "sosvo_dense_wide.h"

namespace {

constexpr int kBig = 1 << 20;       // above any L (<= 64 + 8191) plus P1
constexpr uint32_t kRowBits = 14;   // rows <= 16384: a row index fits 14 bits of the left-right key
constexpr int kDropped = 0xFFFF;    // k* of a pixel without a disparity (255 is a winner at D = 256)

// A lane's W values of C (one byte each) and of S (16 bits each) as one word, slot j in bits 8 j.. and 16 j..
template <int W> struct Packed;
template <> struct Packed<1> { typedef uint8_t C; typedef uint16_t S; };
template <> struct Packed<2> { typedef uint16_t C; typedef uint32_t S; };
template <> struct Packed<4> { typedef uint32_t C; typedef uint64_t S; };

// element index (pixel * D + lane * W) -> the lane's word; the address is a multiple of the word's size (16 | D, W | 16)
template <int W>
__device__ __forceinline__ typename Packed<W>::C load_C(const uint8_t* C, size_t i) {
  return *reinterpret_cast<const typename Packed<W>::C*>(C + i);
}
template <int W>
__device__ __forceinline__ typename Packed<W>::S load_S(const uint16_t* S, size_t i) {
  return *reinterpret_cast<const typename Packed<W>::S*>(S + i);
}
template <int W>
__device__ __forceinline__ void store_C(uint8_t* C, size_t i, const int (&v)[W]) {
  typename Packed<W>::C w = 0;
#pragma unroll
  for (int j = 0; j < W; ++j) w |= (typename Packed<W>::C)((uint32_t)v[j] << (8 * j));
  *reinterpret_cast<typename Packed<W>::C*>(C + i) = w;
}
template <int W>
__device__ __forceinline__ void store_S(uint16_t* S, size_t i, const int (&v)[W]) {
  typename Packed<W>::S w = 0;
#pragma unroll
  for (int j = 0; j < W; ++j) w |= (typename Packed<W>::S)((typename Packed<W>::S)(uint32_t)(v[j] & 0xFFFF) << (16 * j));
  *reinterpret_cast<typename Packed<W>::S*>(S + i) = w;
}
template <int W>
__device__ __forceinline__ int slot_C(typename Packed<W>::C w, int j) { return (int)((w >> (8 * j)) & 0xFF); }
template <int W>
__device__ __forceinline__ int slot_S(typename Packed<W>::S w, int j) { return (int)((w >> (16 * j)) & 0xFFFF); }

// L(p, k) = C(p, k) + min(L_prev(k), L_prev(k - 1) + P1, L_prev(k + 1) + P1, m + P2) - m, m = min_j L_prev(j), for the
// lane's W slots; a lane outside the volume (`in` false) keeps kBig.  k = 0 has no k - 1: lane 0's slot 0.  k = D - 1 has
// no k + 1: its right neighbour is lane 63's entering zero (poisoned here) or a lane outside the volume (kBig already).
template <int W>
__device__ __forceinline__ void sgm_step(const int (&cost)[W], const int (&Lp)[W], int (&L)[W], int P1, int P2, int lane, bool in) {
  int m = Lp[0];
#pragma unroll
  for (int j = 1; j < W; ++j) m = min(m, Lp[j]);
  m = wave_min(m);
  int left = lane_from_left(Lp[W - 1]), right = lane_from_right(Lp[0]);
  left = lane == 0 ? kBig : left;
  right = lane == 63 ? kBig : right;
#pragma unroll
  for (int j = 0; j < W; ++j) {
    const int a = j == 0 ? left : Lp[j == 0 ? 0 : j - 1], b = j == W - 1 ? right : Lp[j == W - 1 ? j : j + 1];
    L[j] = in ? cost[j] + min(min(Lp[j], m + P2), min(a, b) + P1) - m : kBig;
  }
}

// The downward path of column c of frame f (one wave): the costs from the census words, C and S = L written.  Slot j of a
// lane holds the bottom word of row r - d0 - (lane * W + j): every row the words move one slot, one crosses into the next
// lane, and lane 0's slot 0 takes the new one.
template <int W>
__global__ __launch_bounds__(256) void dense_wide_down_kernel(const uint64_t* __restrict__ census_top, const uint64_t* __restrict__ census_bot,
                                                              int rows, int cols, int d0, int D, int P1, int P2, uint8_t* __restrict__ C,
                                                              uint16_t* __restrict__ S) {
  const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= cols) return;  // (the whole wave)
  const bool in = lane * W < D;
  const size_t frame = (size_t)blockIdx.y * rows * cols;
  const uint64_t* ct = census_top + frame + c;
  const uint64_t* cb = census_bot + frame + c;
  uint32_t wlo[W], whi[W];
  int Lp[W];
#pragma unroll
  for (int j = 0; j < W; ++j) {
    wlo[j] = whi[j] = 0;
    Lp[j] = kBig;
  }
  for (int r = 0; r < rows; ++r) {
    const uint32_t in_lo = (uint32_t)lane_from_left((int)wlo[W - 1]), in_hi = (uint32_t)lane_from_left((int)whi[W - 1]);
#pragma unroll
    for (int j = W - 1; j > 0; --j) {
      wlo[j] = wlo[j - 1];
      whi[j] = whi[j - 1];
    }
    wlo[0] = in_lo;
    whi[0] = in_hi;
    const int rb0 = r - d0;
    if (rb0 >= 0) {  // (uniform)
      const uint64_t nw = cb[(size_t)rb0 * cols];
      if (lane == 0) {
        wlo[0] = (uint32_t)nw;
        whi[0] = (uint32_t)(nw >> 32);
      }
    }
    const uint64_t t = ct[(size_t)r * cols];
    int cost[W], L[W];
#pragma unroll
    for (int j = 0; j < W; ++j)
      cost[j] = rb0 - (lane * W + j) >= 0 ? __popc(wlo[j] ^ (uint32_t)t) + __popc(whi[j] ^ (uint32_t)(t >> 32)) : 64;
    if (r == 0) {
#pragma unroll
      for (int j = 0; j < W; ++j) L[j] = in ? cost[j] : kBig;
    } else {
      sgm_step<W>(cost, Lp, L, P1, P2, lane, in);
    }
    if (in) {
      const size_t i = (frame + (size_t)r * cols + c) * D + lane * W;
      store_C<W>(C, i, cost);
      store_S<W>(S, i, L);
    }
#pragma unroll
    for (int j = 0; j < W; ++j) Lp[j] = L[j];
  }
}

// One step of a further path at pixel p: the loaded words of C and S -> S + L stored, Lp replaced.  `first`: L = C.
template <int W>
__device__ __forceinline__ void path_step(typename Packed<W>::C cw, typename Packed<W>::S sw, bool first, int (&Lp)[W], uint16_t* S,
                                          size_t i, int P1, int P2, int lane, bool in) {
  int cost[W], L[W], sum[W];
#pragma unroll
  for (int j = 0; j < W; ++j) cost[j] = slot_C<W>(cw, j);
  if (first) {
#pragma unroll
    for (int j = 0; j < W; ++j) L[j] = in ? cost[j] : kBig;
  } else {
    sgm_step<W>(cost, Lp, L, P1, P2, lane, in);
  }
#pragma unroll
  for (int j = 0; j < W; ++j) {
    sum[j] = slot_S<W>(sw, j) + L[j];
    Lp[j] = L[j];
  }
  if (in) store_S<W>(S, i, sum);
}

// One further path per wave, as dense_path_kernel: line `l` of frame f starts at pixel base + l * line_stride and takes len
// steps of `step` pixels.  C is read, L is added to S.  The next step's words of C and S are in flight while this step's
// recurrence runs (one step ahead: section 37 records eight ahead as a loss).
template <int W>
__global__ __launch_bounds__(256) void dense_wide_path_kernel(const uint8_t* __restrict__ C, uint16_t* __restrict__ S, int nlines, int len,
                                                              long long frame_pixels, long long base, long long line_stride,
                                                              long long step, int D, int P1, int P2) {
  const int lane = threadIdx.x & 63, l = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (l >= nlines) return;  // (the whole wave)
  const bool in = lane * W < D;
  long long p = (long long)blockIdx.y * frame_pixels + base + (long long)l * line_stride;
  typename Packed<W>::C cn = 0;
  typename Packed<W>::S sn = 0;
  if (in) {
    cn = load_C<W>(C, (size_t)p * D + lane * W);
    sn = load_S<W>(S, (size_t)p * D + lane * W);
  }
  int Lp[W];
#pragma unroll
  for (int j = 0; j < W; ++j) Lp[j] = kBig;
  for (int i = 0; i < len; ++i) {
    const typename Packed<W>::C cw = cn;
    const typename Packed<W>::S sw = sn;
    const long long q = p + step;
    if (i + 1 < len && in) {
      cn = load_C<W>(C, (size_t)q * D + lane * W);
      sn = load_S<W>(S, (size_t)q * D + lane * W);
    }
    path_step<W>(cw, sw, i == 0, Lp, S, (size_t)p * D + lane * W, P1, P2, lane, in);
    p = q;
  }
}

// One diagonal path per wave, as dense_diag_kernel: line j of frame f starts in column j of the first
// row (dr = +1) or of the last row (dr = -1) and at every step moves one row by dr and one column by dc, the column wrapping
// modulo cols.  Cyclic: the wrap is the predecessor across the seam.  Clamped: the line starts again with L = C in the column
// it wraps into.  The wave's number is uniform, so the pixel, its column and the wrap are scalar.  One direction per launch:
// two of them in one launch would have two waves read-modify-write the same S.
template <int W, bool kCyclic>
__global__ __launch_bounds__(256) void dense_wide_diag_kernel(const uint8_t* __restrict__ C, uint16_t* __restrict__ S, int rows, int cols,
                                                              int dr, int dc, int D, int P1, int P2) {
  const int lane = threadIdx.x & 63, j0 = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (j0 >= cols) return;  // (the whole wave)
  const bool in = lane * W < D;
  const long long row_step = dr > 0 ? (long long)cols : -(long long)cols;
  const int start_col = dc > 0 ? 0 : cols - 1;  // clamped: where a line starts again
  long long p = (long long)blockIdx.y * rows * cols + (dr > 0 ? 0LL : (long long)(rows - 1) * cols) + j0;
  int c = j0;
  typename Packed<W>::C cn = 0;
  typename Packed<W>::S sn = 0;
  if (in) {
    cn = load_C<W>(C, (size_t)p * D + lane * W);
    sn = load_S<W>(S, (size_t)p * D + lane * W);
  }
  int Lp[W];
#pragma unroll
  for (int j = 0; j < W; ++j) Lp[j] = kBig;
  for (int i = 0; i < rows; ++i) {
    const typename Packed<W>::C cw = cn;
    const typename Packed<W>::S sw = sn;
    int c2 = c + dc;
    long long q = p + row_step + dc;
    if (c2 == cols) {
      c2 = 0;
      q -= cols;
    } else if (c2 < 0) {
      c2 = cols - 1;
      q += cols;
    }
    if (i + 1 < rows && in) {
      cn = load_C<W>(C, (size_t)q * D + lane * W);
      sn = load_S<W>(S, (size_t)q * D + lane * W);
    }
    path_step<W>(cw, sw, i == 0 || (!kCyclic && c == start_col), Lp, S, (size_t)p * D + lane * W, P1, P2, lane, in);
    p = q;
    c = c2;
  }
}

// Winner, uniqueness, reach, mask and the parabola of 64 consecutive pixels per wave, as dense_select_kernel: d16 before the
// left-right check, kstar (0xFFFF = dropped), and with `best` the left-right key (mS << 14 | r) of the bottom row the pixel
// points at.  First lane = W disparities, one pixel after the other: the winner key (S << 8) | k, 24 bits, and the rivals,
// whose results lane j keeps for pixel j.  Then lane = pixel: the two neighbours S(k* - 1), S(k* + 1) are read again from the
// line the wave has just read (they lie in some other lane's slot), then the tests, the division and the stores.
template <int W>
__global__ __launch_bounds__(256) void dense_wide_select_kernel(const uint16_t* __restrict__ S, const uint8_t* __restrict__ mask, int rows,
                                                                int cols, size_t total, int d0, int D, int uniqueness,
                                                                int16_t* __restrict__ d16, uint16_t* __restrict__ kstar,
                                                                uint32_t* __restrict__ best) {
  const int lane = threadIdx.x & 63;
  const size_t first = ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64, frame_pixels = (size_t)rows * cols;
  if (first >= total) return;  // (the whole wave)
  const bool in = lane * W < D;
  const int count = (int)min((size_t)64, total - first);
  int my_key = 0, my_rival = 0;
  for (int j0 = 0; j0 < count; j0 += 8) {
    typename Packed<W>::S sv[8];  // (eight pixels' loads in flight before the first reduction; pixels beyond `count` are not kept)
#pragma unroll
    for (int i = 0; i < 8; ++i) sv[i] = j0 + i < count && in ? load_S<W>(S, (first + j0 + i) * D + lane * W) : 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      int s[W], key = 0x7FFFFFFF;
#pragma unroll
      for (int j = 0; j < W; ++j) {
        s[j] = slot_S<W>(sv[i], j);
        if (in) key = min(key, (s[j] << 8) | (lane * W + j));  // the smallest k among the minimal S
      }
      key = wave_min(key);
      const int ks = key & 255, mS = key >> 8;
      bool rival = false;
#pragma unroll
      for (int j = 0; j < W; ++j) rival = rival || (in && abs(lane * W + j - ks) > 1 && s[j] * (100 - uniqueness) < mS * 100);
      const int any = __ballot(rival) != 0ULL ? 1 : 0;
      if (lane == j0 + i) {
        my_key = key;
        my_rival = any;
      }
    }
  }
  if (lane >= count) return;
  const size_t p = first + lane, pix = p % frame_pixels;
  const int ks = my_key & 255, mS = my_key >> 8;
  const int r = (int)(pix / cols), rb = r - (d0 + ks);
  const bool drop = my_rival != 0 || rb < 0 || (mask && mask[pix] == 0);
  int off = 0;
  if (ks >= 1 && ks <= D - 2) {
    const int a = S[p * D + ks - 1], b = S[p * D + ks + 1];
    const int den = max(a + b - 2 * mS, 1), num = (a - b) * 16 + den;
    off = num >= 0 ? num / (2 * den) : -((-num + 2 * den - 1) / (2 * den));  // floor
  }
  d16[p] = drop ? (int16_t)-1 : (int16_t)((d0 + ks) * 16 + off);
  kstar[p] = drop ? (uint16_t)kDropped : (uint16_t)ks;
  if (best && !drop) atomicMin(best + (p - pix) + (size_t)rb * cols + (pix - (size_t)r * cols), ((uint32_t)mS << kRowBits) | (uint32_t)r);
}

// Left-right, as dense_left_right_kernel with the 16-bit k*
__global__ __launch_bounds__(256) void dense_wide_left_right_kernel(const uint16_t* __restrict__ kstar, const uint32_t* __restrict__ best,
                                                                    int rows, int cols, size_t total, int d0, int lr_max,
                                                                    int16_t* __restrict__ d16) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= total) return;
  const int ks = kstar[p];
  if (ks == kDropped) return;
  const size_t frame_pixels = (size_t)rows * cols, pix = p % frame_pixels;
  const int r = (int)(pix / cols), c = (int)(pix - (size_t)r * cols), rb = r - (d0 + ks);
  const uint32_t key = best[(p - pix) + (size_t)rb * cols + c];  // (written by this pixel at the latest)
  const int kept = kstar[(p - pix) + (size_t)(key & ((1u << kRowBits) - 1)) * cols + c];
  if (abs(kept - ks) > lr_max) d16[p] = -1;
}

struct WideArgs {
  int n, rows, cols, d0, D, P1, P2, uniqueness, lr_max, paths;
  bool cyclic;
  const uint8_t* mask;
  int16_t* d16_out;
};

// The launches of dense_stereo_body with W slots per lane
template <int W>
int32_t run_wide(sosvo_ctx* ctx, const WideArgs& a, const sosvo_dense_wide_scratch& b, uint16_t* S) {
  const int n = a.n, rows = a.rows, cols = a.cols, D = a.D, P1 = a.P1, P2 = a.P2;
  const size_t frame_pixels = (size_t)rows * cols, total = (size_t)n * frame_pixels;
  const bool want_lr = a.lr_max >= 0;
  uint32_t* best = want_lr ? b.best : nullptr;
  SOSVO_LAUNCH_AS(ctx, "dense_wide_down_kernel", dense_wide_down_kernel<W>, dim3(cdiv(cols, 4), n), dim3(256), 0, ctx->stream, b.census_top,
                  b.census_bot, rows, cols, a.d0, D, P1, P2, b.C, S);
  SOSVO_LAUNCH_CHECK(ctx);
  // up: column c from the last row
  SOSVO_LAUNCH_AS(ctx, "dense_wide_path_kernel_up", dense_wide_path_kernel<W>, dim3(cdiv(cols, 4), n), dim3(256), 0, ctx->stream, b.C, S, cols,
                  rows, (long long)frame_pixels, (long long)(rows - 1) * cols, 1LL, -(long long)cols, D, P1, P2);
  SOSVO_LAUNCH_CHECK(ctx);
  // left to right: row r from column 0
  SOSVO_LAUNCH_AS(ctx, "dense_wide_path_kernel_lr", dense_wide_path_kernel<W>, dim3(cdiv(rows, 4), n), dim3(256), 0, ctx->stream, b.C, S, rows,
                  cols, (long long)frame_pixels, 0LL, (long long)cols, 1LL, D, P1, P2);
  SOSVO_LAUNCH_CHECK(ctx);
  // right to left: row r from the last column
  SOSVO_LAUNCH_AS(ctx, "dense_wide_path_kernel_rl", dense_wide_path_kernel<W>, dim3(cdiv(rows, 4), n), dim3(256), 0, ctx->stream, b.C, S, rows,
                  cols, (long long)frame_pixels, (long long)cols - 1, (long long)cols, -1LL, D, P1, P2);
  SOSVO_LAUNCH_CHECK(ctx);
  if (a.paths == 8) {  // the diagonals, one direction per launch
    static const struct { const char* name; int dr, dc; } kDiag[4] = {{"dense_wide_diag_kernel_dr", 1, 1}, {"dense_wide_diag_kernel_dl", 1, -1},
                                                                      {"dense_wide_diag_kernel_ur", -1, 1}, {"dense_wide_diag_kernel_ul", -1, -1}};
    for (const auto& d : kDiag) {
      if (a.cyclic)
        SOSVO_LAUNCH_AS(ctx, d.name, (dense_wide_diag_kernel<W, true>), dim3(cdiv(cols, 4), n), dim3(256), 0, ctx->stream, b.C, S, rows, cols,
                        d.dr, d.dc, D, P1, P2);
      else
        SOSVO_LAUNCH_AS(ctx, d.name, (dense_wide_diag_kernel<W, false>), dim3(cdiv(cols, 4), n), dim3(256), 0, ctx->stream, b.C, S, rows, cols,
                        d.dr, d.dc, D, P1, P2);
      SOSVO_LAUNCH_CHECK(ctx);
    }
  }
  if (want_lr) SOSVO_HIP(ctx, hipMemsetAsync(best, 0xFF, total * 4, ctx->stream));
  SOSVO_LAUNCH_AS(ctx, "dense_wide_select_kernel", dense_wide_select_kernel<W>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                  ctx->stream, S, a.mask, rows, cols, total, a.d0, D, a.uniqueness, a.d16_out, b.kstar, best);
  SOSVO_LAUNCH_CHECK(ctx);
  if (want_lr) {
    SOSVO_LAUNCH(ctx, dense_wide_left_right_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, b.kstar, best, rows,
                 cols, total, a.d0, a.lr_max, a.d16_out);
    SOSVO_LAUNCH_CHECK(ctx);
  }
  return SOSVO_OK;
}

// Scratch, census and the launches for checked arguments, whatever D
int32_t dense_wide_run(sosvo_ctx* ctx, const uint8_t* top, const uint8_t* bot, int32_t n, int32_t rows, int32_t cols, const uint8_t* mask,
                       int32_t min_disparity, int32_t disparities, int32_t P1, int32_t P2, int32_t uniqueness, int32_t lr_max, int32_t flags,
                       int32_t paths, int16_t* d16_out, uint16_t* S_out) {
  const bool cyclic = (flags & SOSVO_DENSE_CYCLIC_COLUMNS) != 0;
  const size_t total = (size_t)n * rows * cols;
  sosvo_dense_wide_scratch b;  // (dense_wide_scratch.h)
  const int32_t rc =
      sosvo_ws_carve(ctx, [&](Carver& cv) { b = sosvo_dense_wide_carve(cv, total, (size_t)disparities, S_out != nullptr, lr_max >= 0); });
  if (rc != SOSVO_OK) return rc;
  int32_t st = sosvo_dense_launch_census(ctx, top, n, rows, cols, cyclic, b.census_top);
  if (st != SOSVO_OK) return st;
  st = sosvo_dense_launch_census(ctx, bot, n, rows, cols, cyclic, b.census_bot);
  if (st != SOSVO_OK) return st;
  const WideArgs a = {n, rows, cols, min_disparity, disparities, P1, P2, uniqueness, lr_max, paths, cyclic, mask, d16_out};
  uint16_t* S = S_out ? S_out : b.S;
  if (disparities <= 64) return run_wide<1>(ctx, a, b, S);
  if (disparities <= 128) return run_wide<2>(ctx, a, b, S);
  return run_wide<4>(ctx, a, b, S);
}

}  // namespace

extern "C" {

int32_t sosvo_dense_stereo_wide(sosvo_ctx* ctx, const uint8_t* top, const uint8_t* bot, int32_t n, int32_t rows, int32_t cols,
                                const uint8_t* mask, int32_t min_disparity, int32_t disparities, int32_t P1, int32_t P2,
                                int32_t uniqueness, int32_t lr_max, int32_t flags, int32_t paths, int16_t* d16_out, uint16_t* S_out) {
  SOSVO_ENTER(ctx);
  const int32_t ok = sosvo_dense_stereo_check(__func__, ctx, top, bot, n, rows, cols, min_disparity, P1, P2, uniqueness, flags, paths, d16_out);
  if (ok != SOSVO_OK) return ok;
  SOSVO_REQUIRE(ctx, disparities >= SOSVO_DENSE_WIDE_MIN_DISPARITIES && disparities <= SOSVO_DENSE_WIDE_MAX_DISPARITIES && disparities % 16 == 0,
                "disparities out of range (16..256, a multiple of 16)");
  if (disparities == SOSVO_DENSE_DISPARITIES)  // dense.hip as it stands: the same launches, the same scratch, the same bytes
    return sosvo_dense_stereo_run64(ctx, top, bot, n, rows, cols, mask, min_disparity, P1, P2, uniqueness, lr_max, flags, paths, d16_out, S_out);
  return dense_wide_run(ctx, top, bot, n, rows, cols, mask, min_disparity, disparities, P1, P2, uniqueness, lr_max, flags, paths, d16_out, S_out);
}

// Test and measurement hook, in no header (as sosvo_debug_fill_scratch is a hook): sosvo_dense_stereo_wide without the
// 64-disparity route, so that these kernels run at D = 64 too, beside dense.hip's (tests/test_gpu_dense_wide.py,
// scripts/bench_dense_wide.py).  The same refusals.
int32_t sosvo_debug_dense_stereo_wide_kernels(sosvo_ctx* ctx, const uint8_t* top, const uint8_t* bot, int32_t n, int32_t rows, int32_t cols,
                                              const uint8_t* mask, int32_t min_disparity, int32_t disparities, int32_t P1, int32_t P2,
                                              int32_t uniqueness, int32_t lr_max, int32_t flags, int32_t paths, int16_t* d16_out,
                                              uint16_t* S_out) {
  SOSVO_ENTER(ctx);
  const int32_t ok = sosvo_dense_stereo_check(__func__, ctx, top, bot, n, rows, cols, min_disparity, P1, P2, uniqueness, flags, paths, d16_out);
  if (ok != SOSVO_OK) return ok;
  SOSVO_REQUIRE(ctx, disparities >= SOSVO_DENSE_WIDE_MIN_DISPARITIES && disparities <= SOSVO_DENSE_WIDE_MAX_DISPARITIES && disparities % 16 == 0,
                "disparities out of range (16..256, a multiple of 16)");
  return dense_wide_run(ctx, top, bot, n, rows, cols, mask, min_disparity, disparities, P1, P2, uniqueness, lr_max, flags, paths, d16_out, S_out);
}

}  // extern "C"
