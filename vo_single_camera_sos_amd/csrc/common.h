// Internal helpers shared by the HIP translation units of libsosvo.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "scratch_carver.h"
#include "sosvo.h"

struct sosvo_prof_entry {
  const char* name;  // string literal
  hipEvent_t a, b;
};

constexpr int kSosvoProfMax = 16384;

constexpr int kSosvoMaxSubStreams = 4;

struct sosvo_ctx {
  int32_t device;
  hipStream_t stream;
  hipEvent_t ev_start, ev_stop;
  char err[512];
  // scratch workspace owned by the context (grown on demand, never inside a capture)
  void* ws;
  size_t ws_bytes;
  // optional per-kernel HIP-event profile (sosvo_profile_*): one event pair per launch
  int32_t prof_on;
  int32_t prof_n;        // entries recorded since the last enable/reset
  int32_t prof_created;  // event pairs that exist
  sosvo_prof_entry* prof;
  // sosvo_frame_pair_batch_streams: internal sub-contexts (own stream, own scratch), created on first use
  sosvo_ctx* sub[kSosvoMaxSubStreams];
  hipEvent_t sub_done[kSosvoMaxSubStreams], sub_median[kSosvoMaxSubStreams], sub_begin;
  int32_t n_sub;
  int32_t hint_score_fp64_only;  // sosvo_set_hint(SOSVO_HINT_SCORE_FP64_ONLY): no single-precision tier in ransac_score_kernel
  int32_t hint_shared_device;  // sosvo_set_hint(SOSVO_HINT_SHARED_DEVICE): other streams' kernels share the chip
  int32_t hint_match_unsplit;  // sosvo_set_hint(SOSVO_HINT_MATCH_UNSPLIT): the matrix-core matchers do not split the train range
  int32_t hint_rolling_narrow;  // sosvo_set_hint(SOSVO_HINT_ROLLING_NARROW): the rolling image kernels in their one-column form
  sosvo_lk_options lk;  // sosvo_set_lk_options: the tracker's settings under SOSVO_FLAG_LK_F2F (cv2's defaults at creation)
  sosvo_stereo_lk_options stereo_lk;  // sosvo_set_stereo_lk_options: the settings of the stage under SOSVO_FLAG_LK_STEREO
  int32_t sub_last;  // parts of the most recent sosvo_frame_pair_batch_streams[_enqueue] call
  // un-joined work of an ..._enqueue call is pending on the part streams: only then does the next call chain its first
  // median behind the previous call's last one, and only then must its slice layout (workspace pointer, part count, each
  // part's bytes) equal the previous one
  int32_t sub_pending;
  const void* sub_last_ws;
  size_t sub_last_bytes[kSosvoMaxSubStreams];
};

// Brackets the kernel launches of the enclosing scope with a HIP event pair when profiling is on.
struct SosvoProfScope {
  sosvo_ctx* ctx;
  bool active;
  SosvoProfScope(sosvo_ctx* c, const char* name) : ctx(c), active(false) {
    if (!c->prof_on || !c->prof || c->prof_n >= kSosvoProfMax) return;
    sosvo_prof_entry& e = c->prof[c->prof_n];
    if (c->prof_n >= c->prof_created) {
      if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) return;
      c->prof_created = c->prof_n + 1;
    }
    e.name = name;
    if (hipEventRecord(e.a, c->stream) != hipSuccess) return;
    active = true;
  }
  ~SosvoProfScope() {
    if (!active) return;
    (void)hipEventRecord(ctx->prof[ctx->prof_n].b, ctx->stream);
    ctx->prof_n++;
  }
};
#define SOSVO_PROFILE(ctx, name) SosvoProfScope sosvo_prof_scope_(ctx, name)

// Kernel launch on the context's stream, labelled `name` in the profile (a kernel picked at run time) ...
#define SOSVO_LAUNCH_AS(ctx, name, kernel, ...) \
  do {                                          \
    SOSVO_PROFILE(ctx, name);                   \
    hipLaunchKernelGGL(kernel, __VA_ARGS__);    \
  } while (0)
// ... and labelled with the kernel's name as it is written.
#define SOSVO_LAUNCH(ctx, kernel, ...) SOSVO_LAUNCH_AS(ctx, #kernel, kernel, __VA_ARGS__)

#define SOSVO_WAVE 64

static inline int32_t sosvo_fail(sosvo_ctx* ctx, int32_t code, const char* what, const char* detail) {
  if (ctx) snprintf(ctx->err, sizeof(ctx->err), "%s: %s", what, detail ? detail : "");
  return code;
}

#define SOSVO_REQUIRE(ctx, cond, msg)                                   \
  do {                                                                  \
    if (!(cond)) return sosvo_fail((ctx), SOSVO_ERR_ARG, __func__, msg); \
  } while (0)

// ... in a file-local body that several entry points share: `fn` is the public function's name
#define SOSVO_REQUIRE_FN(ctx, cond, msg)                           \
  do {                                                             \
    if (!(cond)) return sosvo_fail((ctx), SOSVO_ERR_ARG, fn, msg); \
  } while (0)

// Frames that are read through the unwrap table (sosvo_unwrap_prepare and every consumer of its table): the per-frame
// kernels load 8 bytes at a tap's offset and at that offset + 3 W without a test, and the all-zero entry of a pixel without
// valid taps stands for offset 0, so the 8 bytes from the start of the second row must lie inside the frame.
static inline bool sosvo_table_frame_ok(int64_t H, int64_t W) {
  return H > 0 && W > 0 && H <= 16384 && W <= 16384 && 3 * W * (H - 1) >= 8;
}
#define SOSVO_TABLE_FRAME_MSG \
  "frame size out of range for the unwrap table: 1 <= H, W <= 16384 and 3 * W * (H - 1) >= 8 (8 bytes must follow the start of the second row)"

#define SOSVO_HIP(ctx, call)                                                          \
  do {                                                                                \
    hipError_t e_ = (call);                                                           \
    if (e_ != hipSuccess) return sosvo_fail((ctx), SOSVO_ERR_HIP, #call, hipGetErrorString(e_)); \
  } while (0)

// Every entry point binds the calling thread to the context's device first.
#define SOSVO_ENTER(ctx)                                   \
  do {                                                     \
    if (!(ctx)) return SOSVO_ERR_ARG;                      \
    SOSVO_HIP((ctx), hipSetDevice((ctx)->device));         \
  } while (0)

// Wave priority of the latency-bound kernels: when they share the chip with the VALU-saturating median kernel of another
// stream, their few instructions should issue ahead of its many (s_setprio: arbitration among the waves of a SIMD).
// (measured: +4 % with two streams; 3 for the latency-bound kernels, 2 for the two streaming image kernels, the median 0)
#define SOSVO_LATENCY_BOUND_PRIO() __builtin_amdgcn_s_setprio(3)
#define SOSVO_STREAMING_PRIO() __builtin_amdgcn_s_setprio(2)

#define SOSVO_LAUNCH_CHECK(ctx) SOSVO_HIP((ctx), hipGetLastError())

static inline int32_t sosvo_ws_reserve(sosvo_ctx* ctx, size_t bytes) {
  if (bytes <= ctx->ws_bytes) return SOSVO_OK;
  if (ctx->ws) {
    SOSVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    SOSVO_HIP(ctx, hipFree(ctx->ws));
    ctx->ws = nullptr;
    ctx->ws_bytes = 0;
  }
  SOSVO_HIP(ctx, hipMalloc(&ctx->ws, bytes));
  ctx->ws_bytes = bytes;
  return SOSVO_OK;
}

// A stage's buffers in the context's scratch.  `layout` takes them from a Carver (scratch_carver.h) into the site's
// pointers: it runs over a null base to measure, the total is reserved, and it runs again over ctx->ws as it is AFTER the
// reserve (which may have moved it), so no pointer is ever computed from a stale base.
template <typename Layout>
static inline int32_t sosvo_ws_carve(sosvo_ctx* ctx, Layout layout) {
  Carver measure{nullptr};
  layout(measure);
  const int32_t rc = sosvo_ws_reserve(ctx, measure.off);
  if (rc != SOSVO_OK) return rc;
  Carver place{static_cast<char*>(ctx->ws)};
  layout(place);
  return SOSVO_OK;
}

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// Order-preserving map float -> uint32 (larger float <=> larger uint), for atomicMax and sort keys.
__host__ __device__ static inline uint32_t sosvo_float_ordered(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ static inline float sosvo_ordered_float(uint32_t u) {
  u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

#ifdef __HIPCC__
// Index i of a row / column of n mirrored into [0, n) without repeating the border element (OpenCV's BORDER_REFLECT_101).
__device__ __forceinline__ int refl101(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
  return i;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// nbytes from s to d by the threads i0, i0 + stride, ... of a launch: 16 bytes per lane where both pointers allow it, the
// rest (and everything between unaligned pointers) byte by byte.
__device__ __forceinline__ void sosvo_copy_bytes(uint8_t* __restrict__ d, const uint8_t* __restrict__ s, size_t nbytes, int i0, int stride) {
  size_t done = 0;
  if ((((uintptr_t)d | (uintptr_t)s) & 15) == 0) {
    const size_t nv = nbytes / 16;
    for (size_t i = i0; i < nv; i += stride) reinterpret_cast<uint4*>(d)[i] = reinterpret_cast<const uint4*>(s)[i];
    done = nv * 16;
  }
  for (size_t i = done + i0; i < nbytes; i += stride) d[i] = s[i];
}

// nrows rows of `width` bytes from s (rows s_pitch bytes apart) to d (d_pitch apart) by the threads i0, i0 + stride, ... of a
// launch: 4 bytes per lane where the pointers, the pitches and the width allow it, byte by byte otherwise.
__device__ __forceinline__ void sosvo_copy_rows(uint8_t* __restrict__ d, size_t d_pitch, const uint8_t* __restrict__ s, size_t s_pitch,
                                                int width, int nrows, int i0, int stride) {
  if ((((uintptr_t)d | (uintptr_t)s | d_pitch | s_pitch | (size_t)width) & 3) == 0) {
    const int wq = width / 4;
    for (size_t i = i0; i < (size_t)nrows * wq; i += stride) {
      const size_t r = i / wq, c = i - r * wq;
      reinterpret_cast<uint32_t*>(d + r * d_pitch)[c] = reinterpret_cast<const uint32_t*>(s + r * s_pitch)[c];
    }
    return;
  }
  for (size_t i = i0; i < (size_t)nrows * width; i += stride) {
    const size_t r = i / width, c = i - r * width;
    d[r * d_pitch + c] = s[r * s_pitch + c];
  }
}

// Value of the neighbouring lane through the DPP operand path (wave_shr:1 / wave_shl:1): a VALU move the compiler
// folds into the consuming add/max where it can, instead of a ds_bpermute through the LDS crossbar -- the rolling
// kernels issue 6-10 lane exchanges per row and the LDS pipe, shared by the four SIMDs of a CU, was their limit.
// Lane 0 / 63 receive 0 (they are halo lanes).  Only valid where "neighbouring lane" = "neighbouring column",
// i.e. not in the strips that touch the image border (mirrored columns): those keep the bpermute form.
__device__ __forceinline__ int lane_from_left(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xF, 0xF, true); }
__device__ __forceinline__ int lane_from_right(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x130, 0xF, 0xF, true); }
__device__ __forceinline__ float lane_from_left(float v) { return __int_as_float(lane_from_left(__float_as_int(v))); }
__device__ __forceinline__ float lane_from_right(float v) { return __int_as_float(lane_from_right(__float_as_int(v))); }

// min over the 64 lanes of a non-negative value, in every lane: inside each row of 16 lanes by DPP (two quad
// permutations, row_half_mirror, row_mirror), across the four rows by readlane
__device__ __forceinline__ int wave_min(int v) {
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));   // quad_perm [1, 0, 3, 2]
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));   // quad_perm [2, 3, 0, 1]
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));  // row_half_mirror
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false));  // row_mirror
  return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
             min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// k * x + acc with 24-bit k, x as ONE v_mad_u32_u24, every operand in a VGPR (the compiler multiplies 32-bit values with
// v_mul_lo_u32 and adds separately; __umul24 does not survive its constant folding either).  Integer arithmetic: the
// order of the additions does not matter.
__device__ __forceinline__ uint32_t vmad24(uint32_t k, uint32_t x, uint32_t acc) {
  uint32_t r;
  asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(k), "v"(acc));
  return r;
}

// Stable position of a lane's element among the valid elements of a workgroup round of NW waves (256 threads unless
// said otherwise): wave ballot prefix + running base (*s_running is advanced by the round's total).  wave_off: NW + 1
// ints of LDS.
template <int NW = 4>
__device__ __forceinline__ int sosvo_block_compact_pos(bool valid, int* wave_off, int* s_running, int tid) {
  const int lane = tid & 63, wid = tid >> 6;
  const unsigned long long bal = __ballot(valid);
  __syncthreads();
  if (lane == 0) wave_off[wid + 1] = __popcll(bal);
  __syncthreads();
  if (tid == 0) {
    wave_off[0] = *s_running;
    for (int w = 0; w < NW; ++w) wave_off[w + 1] += wave_off[w];
    *s_running = wave_off[NW];
  }
  __syncthreads();
  return wave_off[wid] + __popcll(bal & ((1ULL << lane) - 1ULL));
}

// Workgroup -> problem (image, mask) for the kernels that run one workgroup per problem and read that image's data (the
// response map around the candidates, the blurred image under the descriptor patches): workgroups are dealt round-robin
// over the 8 XCDs by linear id, so a plain p = blockIdx.x spreads the 12 masks of one image over all eight L2s and
// every L2 fetches the image (measured: 4.1 MB of HBM fetches per pair for 0.84 MB of blurred images; 6.8 MB of pyramid
// fetches per pair in the ORB selection alone).  Here XCD x takes
// the images x, x + 8, x + 16, ... with all their masks: grid = 8 * ceil(nimg / 8) * nmask, -1 for the padding ids.
__device__ __forceinline__ int xcd_problem(int nimg, int nmask) {
  const int xcd = (int)(blockIdx.x & 7), slot = (int)(blockIdx.x >> 3);
  const int img = (slot / nmask) * 8 + xcd, m = slot - (slot / nmask) * nmask;
  return img < nimg ? img * nmask + m : -1;
}
static inline unsigned xcd_grid(int nimg, int nmask) { return (unsigned)(8 * cdiv(nimg, 8) * nmask); }

// len(matches) of one matching problem, for the assemble kernels: how many of its nq 1-NN keys are not SOSVO_KEY_NONE
// (every query's when the train set is not empty; fewer after sosvo_cross_check_matches).  Called by all `threads` threads of
// the workgroup with the same arguments; the result is uniform.
__device__ __forceinline__ int sosvo_block_count_matches(const uint32_t* __restrict__ keys, int nq, int tid, int threads) {
  int kept = 0;
  for (int i0 = 0; i0 < nq; i0 += threads) kept += __syncthreads_count(i0 + tid < nq && keys[i0 + tid] != SOSVO_KEY_NONE);
  return kept;
}
#endif

// dense.hip / dense_speckle.hip: what every dense entry point asks of its frame stack and of its flags (REQ: SOSVO_REQUIRE, or
// SOSVO_REQUIRE_FN in a body that two entry points share)
#define SOSVO_REQUIRE_DENSE_SIZE_AS(REQ, ctx, rows, cols) \
  REQ(ctx, rows >= 1 && rows <= 16384 && cols >= 1 && cols <= 16384, "rows / cols out of range (1..16384)")
#define SOSVO_REQUIRE_DENSE_N_AS(REQ, ctx, n) REQ(ctx, n >= 1 && n <= 32767, "n out of range (1..32767)")
#define SOSVO_REQUIRE_DENSE_FLAGS_AS(REQ, ctx, flags) REQ(ctx, (flags & ~SOSVO_DENSE_CYCLIC_COLUMNS) == 0, "unknown flag bits")
#define SOSVO_REQUIRE_DENSE_SIZE(ctx, rows, cols) SOSVO_REQUIRE_DENSE_SIZE_AS(SOSVO_REQUIRE, ctx, rows, cols)
#define SOSVO_REQUIRE_DENSE_N(ctx, n) SOSVO_REQUIRE_DENSE_N_AS(SOSVO_REQUIRE, ctx, n)
#define SOSVO_REQUIRE_DENSE_FLAGS(ctx, flags) SOSVO_REQUIRE_DENSE_FLAGS_AS(SOSVO_REQUIRE, ctx, flags)

// dense.hip, for dense_wide.hip: what every dense stereo entry point refuses (SOSVO_ERR_ARG under the name `fn`), the census
// launch, and the launches of sosvo_dense_stereo / sosvo_dense_stereo_paths on arguments already checked
int32_t sosvo_dense_stereo_check(const char* fn, sosvo_ctx* ctx, const uint8_t* top, const uint8_t* bot, int32_t n, int32_t rows,
                                 int32_t cols, int32_t min_disparity, int32_t P1, int32_t P2, int32_t uniqueness, int32_t flags,
                                 int32_t paths, const int16_t* d16_out);
int32_t sosvo_dense_launch_census(sosvo_ctx* ctx, const uint8_t* gray, int nimg, int rows, int cols, bool cyclic, uint64_t* out);
int32_t sosvo_dense_stereo_run64(sosvo_ctx* ctx, const uint8_t* top, const uint8_t* bot, int32_t n, int32_t rows, int32_t cols,
                                 const uint8_t* mask, int32_t min_disparity, int32_t P1, int32_t P2, int32_t uniqueness, int32_t lr_max,
                                 int32_t flags, int32_t paths, int16_t* d16_out, uint16_t* S_out);

// detect.hip: the rolling 7x7 blur on images that lie img_stride bytes apart (also used by orb.hip for the pyramid levels)
int32_t sosvo_launch_gauss7(sosvo_ctx* ctx, const uint8_t* in, long long img_stride, int nimg, int rows, int cols,
                            uint8_t* out);
// ... with the output images out_stride bytes apart (level 0 of the ORB pyramid is read from the dense gray batch)
int32_t sosvo_launch_gauss7_to(sosvo_ctx* ctx, const uint8_t* in, long long in_stride, int nimg, int rows, int cols,
                               uint8_t* out, long long out_stride);
// ... restricted to the output rows [row_range[2 v], row_range[2 v + 1]) (device array; v = image / imgs_per_range)
int32_t sosvo_launch_gauss7_rows(sosvo_ctx* ctx, const uint8_t* in, long long in_stride, int nimg, int rows, int cols,
                                 uint8_t* out, long long out_stride, const int32_t* row_range, int imgs_per_range);

// geometry.hip / rgbd.hip: the assemble stages with frame i's record written at record slot_of_frame[i] of the outputs (the
// ..._front_end_slots entry points).  The HOST table travels in kernel arguments, kSosvoSlotArgFrames frames per launch.
constexpr int kSosvoSlotArgFrames = 256;
struct sosvo_slot_table {
  int32_t slot[kSosvoSlotArgFrames];
};
extern "C" {
int32_t sosvo_stereo_assemble_slots(sosvo_ctx* ctx, const sosvo_rig* rig_host, const float* kp_top, const float* kp_bot,
                                    const uint8_t* desc_top, const uint8_t* desc_bot, const int32_t* n_top,
                                    const int32_t* n_bot, const uint32_t* keys, const int32_t* order, int32_t nframes,
                                    const int32_t* slot_of_frame, int32_t nmask, int32_t cap, int32_t out_cap, float* m_top,
                                    float* m_bot, uint8_t* d_top, uint8_t* d_bot, double* X, double* b_top, double* b_bot,
                                    int32_t* M, int32_t* n_cand);
int32_t sosvo_rgbd_assemble_slots(sosvo_ctx* ctx, const sosvo_rgbd_cam* cam_host, const float* kp, const uint8_t* desc,
                                  const int32_t* n, const float* depth, int32_t nframes, const int32_t* slot_of_frame,
                                  int32_t rows, int32_t cols, int32_t cap, int32_t out_cap, float* m, uint8_t* d, double* X,
                                  double* b, int32_t* M);
}

// lk.hip: the gray images of a frame store under SOSVO_FLAG_LK_F2F (pipeline.hip carves them).  Level l is
// [2 * slots, rows_l, cols_l] u8, view-major: image v * slots + s is view v of slot s; rows_{l+1} = (rows_l + 1) / 2.
struct sosvo_lk_images {
  uint8_t* level[SOSVO_LK_MAX_LEVELS];
  int32_t slots, rows, cols;
};
bool sosvo_lk_options_ok(const sosvo_lk_options& o);
bool sosvo_stereo_lk_options_ok(const sosvo_stereo_lk_options& o);
int32_t sosvo_lk_images_fill(sosvo_ctx* ctx, const sosvo_lk_images& im, int32_t levels, const int32_t* row_range, const uint8_t* gray,
                             int32_t nframes, int32_t first_slot, const int32_t* slot_of_frame, bool cyclic = false, int32_t pad = 0);
int32_t sosvo_lk_images_track(sosvo_ctx* ctx, const sosvo_lk_images& im, const sosvo_lk_options& o, const int32_t* row_range,
                              const int32_t* from_img, const int32_t* to_img, int32_t nprob, int32_t cap, const float* pts,
                              const int64_t* store_pt, const int32_t* n, float* next_pts, uint8_t* status, float* err, float* back,
                              bool cyclic = false);
