// K4 -- goodFeaturesToTrack (the reference's default detector) and K6 -- ORB descriptors on given keypoints.
//
//   cv2.goodFeaturesToTrack(pano, maxCorners=N, qualityLevel=0.01, minDistance=5, mask=m, useHarris=False)
//        omnistereo/camera_models.py:1739 (per azimuthal mask), :1778 (no masks), pose_est_tools.py:544 (RGB-D)
//   ORB_create(nfeatures=N).compute(pano, keypoints)     camera_models.py:1765, :1785, pose_est_tools.py:553
//
// Batched over images (view-major) and azimuthal masks; problem p = image * nmask + mask.
//   eig      min-eigenvalue response in float32 with a fixed operation order (identical to the oracle's), the
//            per-mask maximum folded in through an order-preserving atomicMax; the response never goes to memory as a
//            map: the kernel keeps three rows in registers, tests the 3x3 local maximum there and emits the positive
//            local maxima as compact records (value, pixel) into a region of its own per wave;
//   select   one workgroup per problem: the records of the waves that cover the mask's bounding box, thresholded ->
//            sort keys (ordered(value) << 32 | y << 16 | x) in LDS, rank sort (descending value,
//            higher address first), then the greedy minimum-distance pass on an LDS cell grid by the first wave,
//            64 candidates per step with an exact replay of the sequential acceptance rule;
//   blur     7x7 sigma=2 Gaussian in 8.8 fixed point (separable, LDS tile);
//   describe one workgroup per problem: border rule + stable compaction, then one wave per keypoint:
//            lane l evaluates tests l, 64+l, 128+l, 192+l; four 64-bit ballots ARE the 32 descriptor bytes.
// Everything is integer work or float32 with a pinned evaluation order -> bit-exact against the oracle.
#include "common.h"
#include "rolling_layout.h"

#include <type_traits>

namespace {

constexpr int kThreads = 256;
constexpr int kCandCap = 4096;       // candidates kept per (image, mask): 32 KB of LDS sort keys
constexpr int kCandCapSmall = 2048;   // first pass of the two-pass selection: 16 KB of LDS keys, 1536 grid cells
constexpr int kCandCapLarge = 16384; // large-mask variant (whole-image detection, cap > 1024): 128 KB of the 160 KB LDS
constexpr int kMaxMasks = 32;
typedef uint32_t __attribute__((aligned(1))) u32_unaligned;
typedef uint16_t __attribute__((aligned(1))) u16_unaligned;

// ---- K4a: min-eigenvalue map, rolling over rows ---------------------------------------------------------
// One wave owns a 64-column strip (3 halo columns each side, 58 output columns) of one image and walks down a
// chunk of rows; everything a 3x3 Sobel + 3x3 box sum + 3x3 local-maximum test needs from neighbouring columns
// comes from neighbouring LANES (ds_bpermute), everything from neighbouring rows from three-deep register rings.
// Per row and lane: one byte load, ten lane exchanges, ~70 VALU ops; no LDS, no barriers.  Output: per-mask maxima and
// the candidate records -- a candidate of goodFeaturesToTrack is a pixel whose thresholded response is non-zero and
// equals its 3x3 dilation; with 0 < quality < 1 the threshold quality * max is positive wherever a candidate exists (a
// mask whose maximum is <= 0 has none: c > max * q >= max is impossible for c <= max < 0), so exactly the POSITIVE 3x3
// local maxima of the raw response qualify, whatever the threshold turns out to be.  Each wave appends those of its
// (strip, row chunk) to its own region (running position in an SGPR, no atomics, deterministic order); the selection
// kernel applies the threshold once the per-mask maxima are complete.
//   gray row t  -> hd = g[x+1] - g[x-1], hs = g[x-1] + 2 g[x] + g[x+1]                  (integers, exact)
//   P row v=t-1 -> dx = hd(v-1) + 2 hd(v) + hd(v+1), dy = hs(v+1) - hs(v-1), products dx*dx, dx*dy, dy*dy (f32)
//                  and their horizontal 3-sums (a + b) + c in the oracle's order
//   e row y=v-1 -> vertical sums (ha + hc) + hb, min eigenvalue, per-mask maximum, hm = max(e[x-1], e[x], e[x+1])
//   flag row y-1-> e == max(hm(y-2), hm(y-1), hm(y)): 3x3 local maximum; e > 0 and inside some mask -> one record
// Border rules (identical to the tile version it replaces): reflect-101 on the gray image, and a covariance
// product outside the image is the product AT the reflected position.  In x both are "take the mirrored
// lane".  In y a rolling reflect-101 of the gray rows evaluates the Sobel pair of the mirrored row with the
// row order reversed, i.e. dx unchanged and dy negated -- the dx*dy product is negated back (exact).
// Correctly rounded square root of a float that is ZERO OR NORMAL (the sum of two squares of image gradients products: zero
// or above 1e-30, far from the denormal range and from infinity): v_sqrt_f32 is good to one ulp; the result is moved down /
// up by one ulp where the residual says so -- exactly the correction the compiler emits for sqrtf, without its scaling of
// denormal inputs and its class test (7 of its 16 instructions, a seventh of this kernel).  Bit-identical to the host's
// sqrtf on these inputs; the parity tests compare every keypoint.
__device__ __forceinline__ float sqrt_rn_normal(float x) {
  const float s = __builtin_amdgcn_sqrtf(x);
  const float s_dn = __int_as_float(__float_as_int(s) - 1), s_up = __int_as_float(__float_as_int(s) + 1);
  const float r_dn = __builtin_fmaf(-s_dn, s, x), r_up = __builtin_fmaf(-s_up, s, x);
  float r = (r_dn <= 0.0f) ? s_dn : s;
  r = (r_up > 0.0f) ? s_up : r;
  return r;
}

constexpr int kEigHalo = 3;
constexpr int kEigStripW = 64 - 2 * kEigHalo;  // 58

__device__ __forceinline__ void eig_flush(uint32_t* __restrict__ mstat_img, uint32_t bits, uint32_t omax) {
  while (bits) {
    const int m = __ffs(bits) - 1;
    bits &= bits - 1;
    atomicMax(&mstat_img[m * 5], omax);
  }
}

__global__ __launch_bounds__(kThreads) void min_eigen_kernel(const uint8_t* __restrict__ gray,
                                                             const uint32_t* __restrict__ mask_bits, int nimg,
                                                             int images_per_maskset, int rows, int cols, int nmask,
                                                             int strips, int nchunks, int chunk_rows, int wcap,
                                                             uint2* __restrict__ cand, uint32_t* __restrict__ wcnt,
                                                             uint32_t* __restrict__ mstat) {
  SOSVO_STREAMING_PRIO();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * kThreads + threadIdx.x) >> 6));  // in an SGPR: per-image bases become scalar
  if (wave >= nimg * strips * nchunks) return;  // wave-uniform
  const int img = wave / (strips * nchunks);
  const int rem = wave - img * strips * nchunks;
  const int chunk = rem / strips, strip = rem - chunk * strips;
  const int xb = strip * kEigStripW - kEigHalo;  // column of lane 0
  const int xc = xb + lane;
  const int xs = clampi(xc, 0, cols - 1);
  const int ll = clampi(refl101(xs - 1, cols) - xb, 0, 63);  // lane holding column x-1 (mirrored at the border)
  const int lr = clampi(refl101(xs + 1, cols) - xb, 0, 63);
  const bool out_lane = lane >= kEigHalo && lane < 64 - kEigHalo && xc < cols;  // xc >= 0 follows
  // Rows that hold a pixel of some mask of this image's mask set (mask_bbox_kernel, earlier on the stream): only they can
  // own a candidate or feed a per-mask maximum, so the chunk shrinks to them -- their 3x3 neighbourhoods still get the
  // response rows above and below (e_lo / e_hi), which need the gray rows two further out.  With the SOS panoramas the
  // azimuthal masks leave out the elevation padding: about a quarter of the rows.  (wave-uniform, scalar loads)
  uint32_t* mstat_img = mstat + (size_t)img * nmask * 5;
  int r_lo = rows, r_hi = 0;
  {
    const uint32_t* sbb = mstat + (size_t)(img / images_per_maskset) * images_per_maskset * nmask * 5;  // first image of the set
    for (int m = 0; m < nmask; ++m) {
      const uint32_t y1 = sbb[m * 5 + 4];
      if (y1) {
        r_lo = min(r_lo, (int)(0xFFFFFFFFu - sbb[m * 5 + 2]));
        r_hi = max(r_hi, (int)y1);
      }
    }
  }
  const int ys = max(chunk * chunk_rows, r_lo), ye = min(min(rows, chunk * chunk_rows + chunk_rows), r_hi);
  if (ys >= ye) {  // no mask pixel in this chunk: nothing to emit, no maximum to update
    if (lane == 0) wcnt[wave] = 0u;
    return;
  }
  const int e_lo = max(ys - 1, 0), e_hi = min(ye, rows - 1);  // e rows this chunk evaluates
  const int f_lo = max(ys, 1), f_hi = min(ye, rows - 1) - 1;   // flag rows this chunk owns
  const uint8_t* g = gray + (size_t)img * rows * cols;
  uint2* region = cand + (size_t)wave * wcap;  // this wave's candidate records (response, pixel)
  int wpos = 0;                                // records emitted so far (wave-uniform)
  uint32_t mb_prev = 0u;                       // mask word of the row the flag stage looks at (the previous e row)
  const uint32_t* mb = mask_bits + (size_t)(img / images_per_maskset) * rows * cols;
  const uint32_t mask_all = nmask < 32 ? (1u << nmask) - 1u : 0xFFFFFFFFu;
  const float scale = (float)(1.0 / 3060.0);

  // Three-deep register rings indexed by (row mod 3): the row loop is unrolled three times by a fold so that the
  // slot numbers are compile-time constants (no register shuffling); slot P holds the newest row of a phase-P step.
  int hd[3] = {0, 0, 0}, hs[3] = {0, 0, 0};                                          // gray rows t-2, t-1, t
  float pxx[3] = {0.f, 0.f, 0.f}, pxy[3] = {0.f, 0.f, 0.f}, pyy[3] = {0.f, 0.f, 0.f};  // h-sums of P rows v-2, v-1, v
  float hm[3] = {0.f, 0.f, 0.f}, ec[3] = {0.f, 0.f, 0.f};                            // e rows y-2, y-1, y
  uint32_t cur_bits = 0u, cur_max = 0u;
  const int t_first = e_lo - 2, t_last = e_hi + 2;

  // interior strips: the columns x-1 / x+1 of every lane that matters live in lanes -1 / +1
  const bool edge_strip = xb < 1 || xb + 64 > cols - 1;  // wave-uniform
  // The gray rows come three at a time, one ring revolution ahead (round 4, as orb_level_pass_kernel: a wave's rows are `cols`
  // bytes apart -- another cache line every step -- and a load used in the step that issues it leaves the step's whole
  // latency to the other waves of the SIMD).
  int c_cur[3] = {0, 0, 0}, c_pre[3] = {0, 0, 0};
  auto request = [&](int t0) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < 3; ++k) c_pre[k] = (int)g[(uint32_t)(refl101(min(t0 + k, t_last), rows) * cols) + (uint32_t)xs];
  };
  auto step = [&](auto phase_tag, auto edge_tag, const int t) __attribute__((always_inline)) {
    constexpr int P = decltype(phase_tag)::value;
    constexpr bool EDGE = decltype(edge_tag)::value;
    auto left = [&](auto v) { return EDGE ? __shfl(v, ll) : lane_from_left(v); };
    auto right = [&](auto v) { return EDGE ? __shfl(v, lr) : lane_from_right(v); };
    constexpr int i0 = (P + 1) % 3, i1 = (P + 2) % 3, i2 = P;  // slots of rows t-2, t-1, t
    if (t > t_last) return;  // uniform
    // the mask word of the e row this step finishes (y = t - 2) is requested first: its latency hides under the
    // Sobel / box-sum arithmetic below
    const int y_pre = t - 2;
    const bool y_out = y_pre >= ys && y_pre < ye && y_pre >= e_lo && out_lane;
    const uint32_t o_pre = (uint32_t)(max(y_pre, 0) * cols) + (uint32_t)xc;
    const uint32_t mb_pre = y_out ? mb[o_pre] : 0u;
    {
      const int c = c_cur[P];  // gray row t (requested a ring revolution ahead: rows * cols < 2^28)
      const int l = left(c), r = right(c);
      hd[i2] = r - l;
      hs[i2] = (l + 2 * c) + r;
    }
    const int v = t - 1;
    if (v < e_lo - 1) return;  // uniform
    {
      const int dxi = (hd[i0] + 2 * hd[i1]) + hd[i2], dyi = hs[i2] - hs[i0];
      const float dx = (float)dxi * scale, dy = (float)dyi * scale;
      const float xx = dx * dx, yy = dy * dy;
      float xy = dx * dy;
      if (v < 0 || v >= rows) xy = -xy;  // mirrored row: dy came out negated
      pxx[i2] = (left(xx) + xx) + right(xx);
      pxy[i2] = (left(xy) + xy) + right(xy);
      pyy[i2] = (left(yy) + yy) + right(yy);
    }
    const int y = v - 1;
    if (y < e_lo) return;  // uniform
    {
      const float a = ((pxx[i0] + pxx[i1]) + pxx[i2]) * 0.5f, b = (pxy[i0] + pxy[i1]) + pxy[i2];
      const float c = ((pyy[i0] + pyy[i1]) + pyy[i2]) * 0.5f;
      const float e = (a + c) - sqrt_rn_normal(((a - c) * (a - c)) + (b * b));
      if (y_out) {
        const uint32_t bits = mb_pre & mask_all;
        if (bits != cur_bits) {
          eig_flush(mstat_img, cur_bits, cur_max);
          cur_bits = bits;
          cur_max = 0u;
        }
        cur_max = max(cur_max, sosvo_float_ordered(e));
      }
      const float el = left(e), er = right(e);
      hm[i2] = fmaxf(fmaxf(el, e), er);
      ec[i2] = e;
    }
    const int f = y - 1;
    const uint32_t mb_f = mb_prev & mask_all;  // row f was the e row of the previous step
    mb_prev = mb_pre;
    if (f < f_lo || f > f_hi) return;  // uniform
    {
      const float ev = ec[i1];
      const bool is_cand = out_lane && xc >= 1 && xc <= cols - 2 && ev == fmaxf(fmaxf(hm[i0], hm[i1]), hm[i2]) && ev > 0.0f &&
                           mb_f != 0u;
      const unsigned long long bal = __ballot(is_cand);
      if (bal) {  // uniform
        const int pos = wpos + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        if (is_cand && pos < wcap) region[pos] = make_uint2(__float_as_uint(ev), ((uint32_t)f << 16) | (uint32_t)xc);
        wpos += __popcll(bal);
      }
    }
  };
  auto run = [&](auto edge_tag) __attribute__((always_inline)) {
    request(t_first);
    for (int t = t_first; t <= t_last; t += 3) {
#pragma unroll
      for (int k = 0; k < 3; ++k) c_cur[k] = c_pre[k];
      request(t + 3);
      step(std::integral_constant<int, 0>{}, edge_tag, t);
      step(std::integral_constant<int, 1>{}, edge_tag, t + 1);
      step(std::integral_constant<int, 2>{}, edge_tag, t + 2);
    }
  };
  if (edge_strip) run(std::true_type{}); else run(std::false_type{});
  if (lane == 0) wcnt[wave] = (uint32_t)wpos;  // may exceed wcap: the selection kernel reports the overflow
  // per-mask maxima: one set of atomics per wave when all its output lanes saw a single mask word
  const unsigned long long act = __ballot(out_lane && cur_bits != 0u);
  if (act) {
    const int first = __ffsll((long long)act) - 1;
    const uint32_t b0 = __shfl(cur_bits, first);
    if (__ballot(out_lane && cur_bits != 0u && cur_bits != b0) == 0ULL) {
      uint32_t om = (out_lane && cur_bits != 0u) ? cur_max : 0u;
      for (int s = 32; s > 0; s >>= 1) om = max(om, (uint32_t)__shfl_down((int)om, s));
      if (lane == 0) eig_flush(mstat_img, b0, om);
    } else {
      eig_flush(mstat_img, cur_bits, cur_max);
    }
  }
}

// ---- K4a, two columns per lane ---------------------------------------------------------------------------------
// The same walk with lane l holding the columns xb + 2 l (`lo`) and xb + 2 l + 1 (`hi`) of a 128-column span: one gray
// load (a dword that holds the two bytes) and one 8-byte load of the two mask words per row.  A wave owns TWO logical
// strips of kEigWideStripW = 61 outputs (2 x 61 + 6 halo columns = 128): strip 2 sp in the lanes 0 .. 31 (lane 1 hi ..
// lane 31 hi), strip 2 sp + 1 in the lanes 32 .. 63 (lane 32 lo .. lane 62 lo); with an odd strip count the last wave of a
// row of strips owns one.  Regions and their numbering (img * nchunks + chunk) * strips + strip are those of the
// one-column form at this strip width: the wave keeps two running positions and writes two wcnt entries.
//   Neighbours: the left neighbour of a lane's lo pixel is the hi pixel of the lane before it, the right neighbour of its hi
// pixel the lo pixel of the lane after it, the other two are its own -- ten lane moves per row for two pixels.  Every float
// expression is min_eigen_kernel's, association included.
//   Record order inside a region: row-major (rows are walked in order), then ascending x = ascending lane, lo before hi.  A
// candidate's position is the region's running count + the candidates of BOTH ballots (lo and hi) in the lanes below it
// within its half of the wave (v_mbcnt_lo on the low words for the lanes 0 .. 31, v_mbcnt_hi on the high words for the lanes
// 32 .. 63), and a hi candidate follows its own lane's lo candidate.
//   Image border (EDGE instantiation): a lane's two "virtual" columns outside the image load the gray value of their
// reflect-101 mirror image (a mirrored pair is adjacent in memory too, in descending order: the same one load, the bytes
// picked the other way round).  Computed from those, a virtual column's Sobel pair is (-dx, dy) of the mirrored column, exactly (integers, and the float
// conversion and products are sign-symmetric): dx*dx and dy*dy ARE the products at the mirrored position and dx*dy is its
// negative, negated back by a sign flip -- the rule "a product outside the image is the product at the mirrored position"
// with the neighbours still taken from the neighbouring lanes.  In y nothing changes.
//   Loads: the gray row t + 3 and the mask words of the e row t + 1 are requested in step t, a ring revolution before the
// step that reads them, so no step waits on a load it issued itself.

// One v_max_f32, as written: the compiler's fmaxf puts a canonicalising v_max_f32 v, v, v in front of a loop-carried operand it
// cannot prove quiet.  For operands that are never NaN (the only use) the two are the same function.
__device__ __forceinline__ float vmax_f32(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// A wave-uniform pointer into global memory, pinned to a scalar register pair by an empty asm: an address is then (scalar
// base + the lane's 32-bit offset), one v_lshl_add_u64, where the compiler otherwise keeps a 64-bit pointer per lane and adds
// the uniform part to that -- the same instruction count, two VGPRs more, and with them min_eigen_wide_kernel's 80.
typedef const uint8_t __attribute__((address_space(1)))* global_bytes;
typedef unsigned long long __attribute__((aligned(4))) u64_align4;  // two neighbouring 32-bit words
__device__ __forceinline__ global_bytes uniform_global(const void* p) {
  uint64_t u = reinterpret_cast<uint64_t>(p);
  asm("" : "+s"(u));
  return reinterpret_cast<global_bytes>(u);
}

constexpr int kEigWideStripW = 61;
constexpr int kEigWideMinCols = 8;  // below it the one-column form runs (the wide form's border rule needs cols >= 3; 8 as for the blur)

__global__ __launch_bounds__(kThreads) void min_eigen_wide_kernel(const uint8_t* __restrict__ gray,
                                                                  const uint32_t* __restrict__ mask_bits, int nimg,
                                                                  int images_per_maskset, int rows, int cols, int nmask,
                                                                  int strips, int nchunks, int chunk_rows, int wcap,
                                                                  uint2* __restrict__ cand, uint32_t* __restrict__ wcnt,
                                                                  uint32_t* __restrict__ mstat) {
  SOSVO_STREAMING_PRIO();
  const int lane = threadIdx.x & 63;
  const int spairs = (strips + 1) >> 1;
  const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * kThreads + threadIdx.x) >> 6));
  if (wave >= nimg * spairs * nchunks) return;  // wave-uniform
  const int img = wave / (spairs * nchunks);
  const int rem = wave - img * spairs * nchunks;
  const int chunk = rem / spairs, sp = rem - chunk * spairs;
  const int reg_a = (img * nchunks + chunk) * strips + 2 * sp;  // region of the lanes 0 .. 31; reg_a + 1: the lanes 32 .. 63
  const bool has_b = 2 * sp + 1 < strips;                       // (uniform) the second strip exists
  const int xb = sp * (2 * kEigWideStripW) - kEigHalo;          // column of lane 0's lo pixel
  const int x_lo = xb + 2 * lane, x_hi = x_lo + 1;
  // outputs are the columns xb + 3 .. xb + 124 inside the image (x >= 0 follows)
  const bool own_lo = lane >= 2 && lane <= 62 && x_lo < cols, own_hi = lane >= 1 && lane <= 61 && x_hi < cols;
  const bool cd_lo = own_lo && x_lo >= 1 && x_lo <= cols - 2, cd_hi = own_hi && x_hi >= 1 && x_hi <= cols - 2;
  const uint32_t mask_all = nmask < 32 ? (1u << nmask) - 1u : 0xFFFFFFFFu;
  // gray source of the two virtual columns
  auto mirror = [&](int x) { return clampi(x < 0 ? -x : (x >= cols ? 2 * (cols - 1) - x : x), 0, cols - 1); };
  const int m_lo = mirror(x_lo), m_hi = mirror(x_hi);
  // (a dword load at a column clamped into the row, the two bytes picked out of it where they are used: a 16-bit load is
  // zero-extended by an instruction of its own, which the compiler places at the load and with it the wait)
  const int ld_col = clampi(min(m_lo, m_hi), 0, cols - 4);
  const uint32_t src_col = (uint32_t)ld_col;
  const uint32_t sh_lo = 8u * (uint32_t)clampi(m_lo - ld_col, 0, 3), sh_hi = 8u * (uint32_t)clampi(m_hi - ld_col, 0, 3);
  const uint32_t neg_lo = (x_lo < 0 || x_lo >= cols) ? 0x80000000u : 0u, neg_hi = (x_hi < 0 || x_hi >= cols) ? 0x80000000u : 0u;
  uint32_t* mstat_img = mstat + (size_t)img * nmask * 5;
  int r_lo = rows, r_hi = 0;  // rows that hold a pixel of some mask of the image's mask set, as in min_eigen_kernel
  {
    const uint32_t* sbb = mstat + (size_t)(img / images_per_maskset) * images_per_maskset * nmask * 5;
    for (int m = 0; m < nmask; ++m) {
      const uint32_t y1 = sbb[m * 5 + 4];
      if (y1) {
        r_lo = min(r_lo, (int)(0xFFFFFFFFu - sbb[m * 5 + 2]));
        r_hi = max(r_hi, (int)y1);
      }
    }
  }
  const int ys = max(chunk * chunk_rows, r_lo), ye = min(min(rows, chunk * chunk_rows + chunk_rows), r_hi);
  if (ys >= ye) {
    if (lane == 0) {
      wcnt[reg_a] = 0u;
      if (has_b) wcnt[reg_a + 1] = 0u;
    }
    return;
  }
  const int e_lo = max(ys - 1, 0), e_hi = min(ye, rows - 1);
  const int f_lo = max(ys, 1), f_hi = min(ye, rows - 1) - 1;
  const uint8_t* g = gray + (size_t)img * rows * cols;
  uint2* region = cand + (size_t)(reg_a + (lane >> 5)) * wcap;  // the lane's region
  int wpos_a = 0, wpos_b = 0;                                  // records emitted so far (wave-uniform)
  const uint32_t* mb = mask_bits + (size_t)(img / images_per_maskset) * rows * cols;
  const float scale = (float)(1.0 / 3060.0);

  // The rings start unset: a stage first runs once the three rows it reads are written (the P stage from the third step on,
  // after three gray rows; the e stage two steps later, after three P rows; the flag stage from f_lo = e_lo + 1 on, after the
  // e rows e_lo .. e_lo + 2), so no slot is read before a step wrote it and no register is cleared for nothing.
  int hd_l[3], hs_l[3], hd_h[3], hs_h[3];
  float pxx_l[3], pxy_l[3], pyy_l[3], pxx_h[3], pxy_h[3], pyy_h[3];
  float hm_l[3], ec_l[3], hm_h[3], ec_h[3];
  // Running per-mask maximum of the lo / hi column: the mask word of the current run and the largest response under it AS A
  // FLOAT (one v_max_f32 per pixel and row); the ordered key that mstat holds is made where a run is flushed.  Exact: a
  // response here is finite -- the products are bounded by (4 * 255 / 3060)^2 and sqrt_rn_normal gets a sum of two squares,
  // so no operand is ever NaN or infinite -- and never -0.0 (a + c is a sum of halved sums of squares, >= +0, and x - y
  // with x, y >= +0 rounds to +0 when it is zero), so two responses that compare equal have the same bits and
  // sosvo_float_ordered, strictly increasing on such values, commutes with the maximum.  A run starts at -inf (key
  // 0x007FFFFF, below every response's) and takes a response in the same step; a run under the word 0 is never flushed.
  // The word of the running run IS the mask word of the previous e row (a run ends where the word changes), which is also
  // the row the flag stage looks at: the words live in a ring indexed by phase like the others, mk_*[slot of row y], and
  // nothing is handed over from step to step.  Words are kept for every lane (cleared outside the rows ys .. ye - 1 only);
  // a lane outside the output columns is cleared where a run is flushed, and cd_* keeps it out of the flag stage.
  uint32_t mk_l[3] = {0u, 0u, 0u}, mk_h[3] = {0u, 0u, 0u};
  float max_l = -__builtin_inff(), max_h = -__builtin_inff();
  const int t_first = e_lo - 2, t_last = e_hi + 2;
  const bool edge_strip = xb < 0 || xb + 128 > cols;  // wave-uniform: some lane's column is outside the image
  // mask-word columns: the lane's own ones where they lie inside the image (as byte offsets into a row of mask words)
  const uint32_t mo_lo = 4u * (uint32_t)clampi(x_lo, 0, cols - 1), mo_hi = 4u * (uint32_t)clampi(x_hi, 0, cols - 1);
  // The sign rules as factors: a mirrored row negates dy and a mirrored column dx, and the dx * dy product is negated back.
  // IEEE multiplication is symmetric in sign, so scaling dy (dx) by -scale gives exactly -dy (-dx): the squares keep their
  // bits and dx * dy comes out as the negated product, signed zeros included -- the same values as negating the product.
  const unsigned long long cdb_lo = __builtin_amdgcn_ballot_w64(cd_lo), cdb_hi = __builtin_amdgcn_ballot_w64(cd_hi);
  const float sx_lo = __uint_as_float(__float_as_uint(scale) ^ neg_lo), sx_hi = __uint_as_float(__float_as_uint(scale) ^ neg_hi);
  // Prefetch slots, indexed by phase like the rings: step t reads slot t mod 3 and then refills it for step t + 3, so the
  // value a step reads is in the register the step three before it loaded into -- no hand-over copies.
  // (All three are requested before the first step.)
  uint32_t c_pre[3], mw_l[3], mw_h[3];
  auto request = [&](auto slot_tag, auto edge_tag, const int t) __attribute__((always_inline)) {  // row t -> slot t mod 3
    constexpr int P = decltype(slot_tag)::value;
    constexpr bool EDGE = decltype(edge_tag)::value;
    c_pre[P] = *reinterpret_cast<const u32_unaligned*>(g + ((uint32_t)(refl101(min(t, t_last), rows) * cols) + src_col));
    // the mask words of the e row that step t finishes, y = t - 2: always loaded, from a row clamped into the image; the
    // step clears the words of a row outside ys .. ye - 1 (the few rows a chunk steps over before ys and after ye - 1), so no slot is zeroed here
    // (the row's base is uniform, held in a scalar pair; the lane's byte offset is constant: one 64-bit add per load)
    const global_bytes mrow = uniform_global(mb + (uint32_t)(clampi(t - 2, 0, rows - 1) * cols));
    if (EDGE) {
      mw_l[P] = *reinterpret_cast<const uint32_t __attribute__((address_space(1)))*>(mrow + mo_lo);
      mw_h[P] = *reinterpret_cast<const uint32_t __attribute__((address_space(1)))*>(mrow + mo_hi);
    } else {  // all 128 columns lie inside the image: x_lo >= 0, x_hi <= cols - 1
      const unsigned long long w = *reinterpret_cast<const u64_align4 __attribute__((address_space(1)))*>(mrow + mo_lo);
      mw_l[P] = (uint32_t)w;
      mw_h[P] = (uint32_t)(w >> 32);
    }
  };
  auto eig = [&](float xx0, float xx1, float xx2, float xy0, float xy1, float xy2, float yy0, float yy1, float yy2) {
    const float a = ((xx0 + xx1) + xx2) * 0.5f, b = (xy0 + xy1) + xy2;
    const float c = ((yy0 + yy1) + yy2) * 0.5f;
    return (a + c) - sqrt_rn_normal(((a - c) * (a - c)) + (b * b));
  };
  // One row step; false once t is past the last row (the caller leaves the loop: nothing of the rings or the prefetch slots
  // is live after it, so the ragged tail costs the steady loop no merge).
  auto step = [&](auto phase_tag, auto edge_tag, const int t) __attribute__((always_inline)) {
    constexpr int P = decltype(phase_tag)::value;
    constexpr bool EDGE = decltype(edge_tag)::value;
    constexpr int i0 = (P + 1) % 3, i1 = (P + 2) % 3, i2 = P;  // slots of rows t-2, t-1, t
    if (t > t_last) return false;  // uniform
    const int y = t - 2;           // the e row this step finishes
    const uint32_t c = c_pre[P];
    const int cl = (int)((c >> sh_lo) & 0xFFu), ch = (int)((c >> sh_hi) & 0xFFu);
    const uint32_t row_all = (y >= ys && y < ye) ? mask_all : 0u;  // uniform
    mk_l[i2] = mw_l[P] & row_all;                                  // mask words of the e row
    mk_h[i2] = mw_h[P] & row_all;
    request(phase_tag, edge_tag, t + 3);  // (after the slot's last read)
    {
      const int l = lane_from_left(ch), r = lane_from_right(cl);
      hd_l[i2] = ch - l;
      hs_l[i2] = (l + 2 * cl) + ch;
      hd_h[i2] = r - cl;
      hs_h[i2] = (cl + 2 * ch) + r;
    }
    const int v = t - 1;
    if (v < e_lo - 1) return true;  // uniform
    {
      // mirrored row (v < 0 or v > rows - 1; uniform, so the sign is made by scalar integer instructions): dy comes out negated
      const float sy = __uint_as_float(__float_as_uint(scale) ^ ((uint32_t)(v | (rows - 1 - v)) & 0x80000000u));
      const float dx_l = (float)((hd_l[i0] + 2 * hd_l[i1]) + hd_l[i2]) * (EDGE ? sx_lo : scale), dy_l = (float)(hs_l[i2] - hs_l[i0]) * sy;
      const float dx_h = (float)((hd_h[i0] + 2 * hd_h[i1]) + hd_h[i2]) * (EDGE ? sx_hi : scale), dy_h = (float)(hs_h[i2] - hs_h[i0]) * sy;
      const float xx_l = dx_l * dx_l, yy_l = dy_l * dy_l, xx_h = dx_h * dx_h, yy_h = dy_h * dy_h;
      const float xy_l = dx_l * dy_l, xy_h = dx_h * dy_h;
      pxx_l[i2] = (lane_from_left(xx_h) + xx_l) + xx_h;
      pxx_h[i2] = (xx_l + xx_h) + lane_from_right(xx_l);
      pxy_l[i2] = (lane_from_left(xy_h) + xy_l) + xy_h;
      pxy_h[i2] = (xy_l + xy_h) + lane_from_right(xy_l);
      pyy_l[i2] = (lane_from_left(yy_h) + yy_l) + yy_h;
      pyy_h[i2] = (yy_l + yy_h) + lane_from_right(yy_l);
    }
    if (y < e_lo) return true;  // uniform
    {
      const float e_l = eig(pxx_l[i0], pxx_l[i1], pxx_l[i2], pxy_l[i0], pxy_l[i1], pxy_l[i2], pyy_l[i0], pyy_l[i1], pyy_l[i2]);
      const float e_h = eig(pxx_h[i0], pxx_h[i1], pxx_h[i2], pxy_h[i0], pxy_h[i1], pxy_h[i2], pyy_h[i0], pyy_h[i1], pyy_h[i2]);
      // per-mask maximum: a mask word is 0 outside the rows ys .. ye - 1, and a run under the word 0 is never flushed
      if (mk_l[i2] != mk_l[i1]) {
        eig_flush(mstat_img, own_lo ? mk_l[i1] : 0u, sosvo_float_ordered(max_l));
        max_l = -__builtin_inff();
      }
      max_l = vmax_f32(max_l, e_l);
      if (mk_h[i2] != mk_h[i1]) {
        eig_flush(mstat_img, own_hi ? mk_h[i1] : 0u, sosvo_float_ordered(max_h));
        max_h = -__builtin_inff();
      }
      max_h = vmax_f32(max_h, e_h);
      hm_l[i2] = fmaxf(fmaxf(lane_from_left(e_h), e_l), e_h);
      hm_h[i2] = fmaxf(fmaxf(e_l, e_h), lane_from_right(e_l));
      ec_l[i2] = e_l;
      ec_h[i2] = e_h;
    }
    const int f = y - 1;
    if (f < f_lo || f > f_hi) return true;  // uniform
    {
      const float ev_l = ec_l[i1], ev_h = ec_h[i1];
      // row f was the e row of the previous step (slot i1).  Each predicate goes to a ballot of its own (a compare that
      // writes the lane mask) and the masks are combined as scalars: no predicate is materialised as 0 / 1 on the way.
      const float m3_l = fmaxf(fmaxf(hm_l[i0], hm_l[i1]), hm_l[i2]), m3_h = fmaxf(fmaxf(hm_h[i0], hm_h[i1]), hm_h[i2]);
      const unsigned long long bal_l = cdb_lo & __builtin_amdgcn_ballot_w64(ev_l == m3_l) & __builtin_amdgcn_ballot_w64(ev_l > 0.0f) &
                                       __builtin_amdgcn_ballot_w64(mk_l[i1] != 0u);
      const unsigned long long bal_h = cdb_hi & __builtin_amdgcn_ballot_w64(ev_h == m3_h) & __builtin_amdgcn_ballot_w64(ev_h > 0.0f) &
                                       __builtin_amdgcn_ballot_w64(mk_h[i1] != 0u);
      if (bal_l | bal_h) {  // uniform
        const bool is_l = (bal_l >> lane) & 1ull, is_h = (bal_h >> lane) & 1ull;
        const uint32_t al = (uint32_t)bal_l, ah = (uint32_t)bal_h, bl = (uint32_t)(bal_l >> 32), bh = (uint32_t)(bal_h >> 32);
        const int below_a = (int)__builtin_amdgcn_mbcnt_lo(al, __builtin_amdgcn_mbcnt_lo(ah, 0u));  // lanes 0 .. 31
        const int below_b = (int)__builtin_amdgcn_mbcnt_hi(bl, __builtin_amdgcn_mbcnt_hi(bh, 0u));  // lanes 32 .. 63 (0 below them)
        const int pos_l = lane < 32 ? wpos_a + below_a : wpos_b + below_b, pos_h = pos_l + (is_l ? 1 : 0);
        if (is_l && pos_l < wcap) region[pos_l] = make_uint2(__float_as_uint(ev_l), ((uint32_t)f << 16) | (uint32_t)x_lo);
        if (is_h && pos_h < wcap) region[pos_h] = make_uint2(__float_as_uint(ev_h), ((uint32_t)f << 16) | (uint32_t)x_hi);
        wpos_a += __popc(al) + __popc(ah);
        wpos_b += __popc(bl) + __popc(bh);
      }
    }
    return true;
  };
  uint32_t bits_l = 0u, bits_h = 0u;  // words of the runs still open after the last row
  auto run = [&](auto edge_tag) __attribute__((always_inline)) {
    request(std::integral_constant<int, 0>{}, edge_tag, t_first);
    request(std::integral_constant<int, 1>{}, edge_tag, t_first + 1);
    request(std::integral_constant<int, 2>{}, edge_tag, t_first + 2);
    int last = 2;  // slot of the last row stepped: where the running runs' words are
    for (int t = t_first;; t += 3) {
      if (!step(std::integral_constant<int, 0>{}, edge_tag, t)) break;
      last = 0;
      if (!step(std::integral_constant<int, 1>{}, edge_tag, t + 1)) break;
      last = 1;
      if (!step(std::integral_constant<int, 2>{}, edge_tag, t + 2)) break;
      last = 2;
    }
    bits_l = last == 0 ? mk_l[0] : (last == 1 ? mk_l[1] : mk_l[2]);
    bits_h = last == 0 ? mk_h[0] : (last == 1 ? mk_h[1] : mk_h[2]);
  };
  if (edge_strip) run(std::true_type{}); else run(std::false_type{});
  if (lane == 0) {  // may exceed wcap: the selection kernel reports the overflow
    wcnt[reg_a] = (uint32_t)wpos_a;
    if (has_b) wcnt[reg_a + 1] = (uint32_t)wpos_b;
  }
  // per-mask maxima: one set of atomics per wave and column parity when all its lanes saw a single mask word
  auto finish = [&](uint32_t cur_bits, uint32_t cur_max) __attribute__((always_inline)) {
    const unsigned long long act = __ballot(cur_bits != 0u);
    if (act) {
      const int first = __ffsll((long long)act) - 1;
      const uint32_t b0 = __shfl(cur_bits, first);
      if (__ballot(cur_bits != 0u && cur_bits != b0) == 0ULL) {
        uint32_t om = cur_bits != 0u ? cur_max : 0u;
        for (int s = 32; s > 0; s >>= 1) om = max(om, (uint32_t)__shfl_down((int)om, s));
        if (lane == 0) eig_flush(mstat_img, b0, om);
      } else {
        eig_flush(mstat_img, cur_bits, cur_max);
      }
    }
  };
  finish(own_lo ? bits_l : 0u, sosvo_float_ordered(max_l));
  finish(own_hi ? bits_h : 0u, sosvo_float_ordered(max_h));
}

// Bounding box of every mask of every mask set (depends on the masks only): mstat fields 1..4 of the FIRST
// image of the set, each grown by atomicMax: 0xFFFFFFFF - xmin, 0xFFFFFFFF - ymin, xmax + 1, ymax + 1.
__global__ __launch_bounds__(kThreads) void mask_bbox_kernel(const uint32_t* __restrict__ mask_bits, int images_per_maskset,
                                                             int rows, int cols, int nmask, uint32_t* __restrict__ mstat) {
  __shared__ uint32_t sb[2][kMaxMasks];
  const int tid = threadIdx.x, y = blockIdx.x, set = blockIdx.y;
  if (tid < 2 * kMaxMasks) (&sb[0][0])[tid] = 0u;
  __syncthreads();
  const uint32_t* mb = mask_bits + ((size_t)set * rows + y) * cols;
  const uint32_t mask_all = nmask < 32 ? (1u << nmask) - 1u : 0xFFFFFFFFu;
  for (int x = tid; x < cols; x += kThreads) {
    uint32_t b = mb[x] & mask_all;
    while (b) {
      const int m = __ffs(b) - 1;
      b &= b - 1;
      atomicMax(&sb[0][m], 0xFFFFFFFFu - (uint32_t)x);
      atomicMax(&sb[1][m], (uint32_t)x + 1u);
    }
  }
  __syncthreads();
  if (tid < nmask && sb[1][tid]) {
    uint32_t* st = mstat + ((size_t)set * images_per_maskset * nmask + tid) * 5;
    atomicMax(&st[1], sb[0][tid]);
    atomicMax(&st[2], 0xFFFFFFFFu - (uint32_t)y);
    atomicMax(&st[3], sb[1][tid]);
    atomicMax(&st[4], (uint32_t)y + 1u);
  }
}

// LOGR consecutive steps of a bitonic merge (strides jtop, jtop / 2, ...) on 2^LOGR keys per thread: the keys
// i + m * jl (jl = the lowest stride) form a closed set under those steps, and they share the merge direction (bit k of i).
template <int LOGR, int NT>
__device__ __forceinline__ void bitonic_pass(unsigned long long* keys, int N, int k, int jtop, int tid) {
  constexpr int R = 1 << LOGR;
  const int jl = jtop >> (LOGR - 1);
  for (int t = tid; t < (N >> LOGR); t += NT) {
    const int i = ((t & ~(jl - 1)) << LOGR) | (t & (jl - 1));
    const bool desc = (i & k) == 0;
    unsigned long long v[R];
#pragma unroll
    for (int m = 0; m < R; ++m) v[m] = keys[i + m * jl];
#pragma unroll
    for (int sb = LOGR - 1; sb >= 0; --sb) {
#pragma unroll
      for (int m = 0; m < R; ++m) {
        if (m & (1 << sb)) continue;
        const unsigned long long a = v[m], b = v[m | (1 << sb)];
        const bool sw = (a < b) == desc;
        v[m] = sw ? b : a;
        v[m | (1 << sb)] = sw ? a : b;
      }
    }
#pragma unroll
    for (int m = 0; m < R; ++m) keys[i + m * jl] = v[m];
  }
}

// One workgroup per problem (image, mask).  Phase 1 gathers the candidate records of the waves of min_eigen_kernel whose
// (strip, row chunk) meets the mask's bounding box (region counts fetched NT at a time, the waves share the regions, one
// LDS atomic per wave and 64 records), keeps those of this mask above the threshold and builds the sort keys in LDS; phase 2
// sorts them (bitonic, descending value, higher address first; three steps per pass over the keys); phase 3 -- the keys are
// dead, their LDS becomes the cell grid -- is the greedy minimum-distance pass, 64 candidates per round: the candidates are
// tested against the grid of already accepted points (9 cells x 2 slots) and against each other (a 64 x 64 conflict matrix),
// both spread over the workgroup's waves, and the first wave then replays the sequential acceptance rule exactly (accept iff
// no conflict with anything accepted before) -- in parallel for the candidates nothing earlier in the round can touch, on
// the scalar unit for the few others.  Round 3: 566 -> ~190 us per whole-image problem of 8 k candidates / 2000 corners
// (region walk 223 -> 25, sort 104 -> 84, greedy 234 -> 70).
// (NT threads per workgroup: 256, or 1024 for the whole-image variant whose 128 KB of LDS allow one workgroup per CU anyway)
// Squared distance of two points packed as y << 16 | x (coordinates below 32768): v_pk_sub_i16 + v_dot2_i32_i16
__device__ __forceinline__ uint32_t dist2_packed(uint32_t a, uint32_t b) {
  typedef short short2v __attribute__((ext_vector_type(2)));
  const short2v d = __builtin_bit_cast(short2v, a) - __builtin_bit_cast(short2v, b);
  return (uint32_t)__builtin_amdgcn_sdot2(d, d, 0, false);
}

// The integer form of the greedy pass's cell grid, shared by its spread and its one-wave form: a one-cell border around the
// cells of the mask's bounding box (no bounds tests on the nine neighbours), two slots of packed coordinates per cell, empty
// slots = kGridEmpty, a third point of a cell in the overflow list.  Holds when min_distance >= 1, cell <= 2048 and rows,
// cols <= 32768: squared distances below 2^31, thresholds below 2^24, so the integer comparisons are the float ones exactly.
constexpr uint32_t kGridEmpty = 0xFFFFFFFFu;
struct gft_igrid {
  uint32_t thr_i;  // integer d2 < md2  <=>  d2 < ceil(md2)
  uint32_t magic;  // v / cell = mulhi(v, magic) for v < 2^16 (cell > 1)
  int cell, cx0, cy0, gwp;
  __device__ __forceinline__ gft_igrid(float md2, int cell_, int cx0_, int cy0_, int gwp_)
      : thr_i((uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)ceilf(md2))),  // (uniform, but out of the VALU: to SGPRs)
        magic((uint32_t)__builtin_amdgcn_readfirstlane((int)(cell_ > 1 ? 0xFFFFFFFFu / (uint32_t)cell_ + 1u : 0u))), cell(cell_),
        cx0(cx0_), cy0(cy0_), gwp(gwp_) {}
  // first slot of the cell of a candidate (every candidate of a mask lies inside the mask's bounding box); an idle lane
  // gets cell (1, 1), which exists
  __device__ __forceinline__ int cell_index(uint32_t xy, bool active) const {
    const uint32_t x = xy & 0xFFFFu, y = xy >> 16;
    const int xc = active ? (int)(cell > 1 ? __umulhi(x, magic) : x) - cx0 + 1 : 1;
    const int yc = active ? (int)(cell > 1 ? __umulhi(y, magic) : y) - cy0 + 1 : 1;
    return (yc * gwp + xc) * 2;
  }
  // does a point of the neighbour cell (dxc, dyc in -1 .. 1 around cidx) lie closer than min_distance to xy?
  __device__ __forceinline__ uint32_t cell_hit(const uint32_t* grid, int cidx, int dxc, int dyc, uint32_t xy) const {
    const uint2 q2 = *reinterpret_cast<const uint2*>(&grid[cidx + dyc * gwp * 2 + dxc * 2]);
    return ((uint32_t)(q2.x != kGridEmpty) & (uint32_t)(dist2_packed(xy, q2.x) < thr_i)) |
           ((uint32_t)(q2.y != kGridEmpty) & (uint32_t)(dist2_packed(xy, q2.y) < thr_i));
  }
  __device__ __forceinline__ bool near(uint32_t a, uint32_t b) const { return dist2_packed(a, b) < thr_i; }
  // an accepted point enters its cell.  A cell of round(minDistance) pixels holds two points -- or, from a distance of ~30
  // pixels on, three in a triangle: the third goes to the overflow list every candidate is tested against (an overflow of
  // that list is reported once, after the loop, from s_ovf)
  __device__ __forceinline__ void insert(uint32_t* grid, int cidx, uint32_t xy, int* s_ovf, uint32_t* acc_list, int limit_list) const {
    if (atomicCAS(&grid[cidx], kGridEmpty, xy) != kGridEmpty && atomicCAS(&grid[cidx + 1], kGridEmpty, xy) != kGridEmpty) {
      const int o = atomicAdd(s_ovf, 1);
      if (o < limit_list) acc_list[o] = xy;
    }
  }
};

// The candidate records carry their pixel as y << 16 | x (rows, cols <= 65535), and so do the sort keys (ordered response
// << 32 | y << 16 | x).  For x < cols <= 65535 the order of (y << 16 | x) is the lexicographic order of (y, x), which is the
// order of the linear address y * cols + x: among equal responses "higher address first" picks the same candidate, the
// keys stay unique, and the CAND largest keys of the overflow path are the same set -- every output is what the linear keys
// gave.  The mask word of a record is one multiply-add away (y * cols + x); nothing divides by cols any more.
//
// The candidate regions of one problem (what phase 1 of gft_select_kernel walks), for the overflow path below.
struct gft_regions {
  const uint2* cand;
  const uint32_t* wcnt;
  const uint32_t* mb;
  int img, m, cols, strips, nchunks, wcap, s0, c0, ns, R;
  float thr;
};

// Every sort key of the problem (the records of this mask above the threshold), one call of f per key and lane, the
// regions NT at a time as in phase 1.  Ends with a barrier.
template <int NT, class F>
__device__ __forceinline__ void gft_walk_keys(const gft_regions& g, int* s_region, int tid, F&& f) {
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  for (int rb = 0; rb < g.R; rb += NT) {
    if (rb + tid < g.R) {
      const int rg = rb + tid, c = g.c0 + rg / g.ns, sidx = g.s0 + rg % g.ns;
      s_region[tid] = min((int)g.wcnt[(g.img * g.nchunks + c) * g.strips + sidx], g.wcap);
    }
    __syncthreads();
    const int rend = min(NT, g.R - rb);
    for (int rr = wave; rr < rend; rr += NT / 64) {
      const int have = s_region[rr];
      const int rg = rb + rr, c = g.c0 + rg / g.ns, sidx = g.s0 + rg % g.ns;
      const uint2* region = g.cand + (size_t)((g.img * g.nchunks + c) * g.strips + sidx) * g.wcap;
      for (int i = lane; i < have; i += 64) {
        const uint2 r = region[i];
        if (__uint_as_float(r.x) > g.thr && ((g.mb[(r.y >> 16) * (uint32_t)g.cols + (r.y & 0xFFFFu)] >> g.m) & 1u))
          f(((unsigned long long)sosvo_float_ordered(__uint_as_float(r.x)) << 32) | r.y);
      }
    }
    __syncthreads();  // s_region is rewritten by the next tile
  }
}

// More candidates than the selection sorts (total > CAND, uniform): the kept set is the CAND LARGEST keys.  The keys
// (ordered response << 32 | y << 16 | x) are unique, so that set -- and with it kp, n and their order -- depends on the image, the
// mask and the parameters only, and the greedy pass on it gives a prefix of the unlimited result.  A radix select finds the
// CAND-th largest key: one more walk over the regions per 11-bit digit with a histogram in the key LDS (which holds
// nothing worth keeping at this point), from the top digit down, until every key left under the digits found so far is
// kept -- three walks when the responses around the cut differ, up to six when the cut lies inside a run of equal responses
// and the address decides.  A last walk gathers the keys >= that cutoff (in any order: the sort follows).  Inlined
// into the one uniform branch that calls it (as a call it raised the kernel's register count from 34 to 72-84 and cost the
// 256-thread variant three of its eight waves per SIMD; inlined the count is 42 and the occupancy unchanged), and that
// branch is marked unlikely so that its code lies behind the usual path, not in the middle of it.
template <int CAND, int NT>
__device__ __forceinline__ void gft_keep_largest(const gft_regions g, unsigned long long* keys, int* s_region, int* s_count,
                                              int* s_sel, int tid) {
  constexpr int kBits = 11, kBins = 1 << kBits, kPer = kBins / 64;
  static_assert(kBins * sizeof(uint32_t) <= CAND * sizeof(unsigned long long), "the histogram lives in the key LDS");
  uint32_t* hist = reinterpret_cast<uint32_t*>(keys);
  unsigned long long prefix = 0ULL;  // the digits of the cutoff found so far, in place
  int want = CAND;                   // rank of the cutoff among the keys that share those digits
  for (int shift = 64; shift > 0;) {
    const int width = min(kBits, shift);
    const unsigned long long high = shift < 64 ? ~0ULL << shift : 0ULL;
    shift -= width;
    for (int i = tid; i < kBins; i += NT) hist[i] = 0u;
    __syncthreads();
    gft_walk_keys<NT>(g, s_region, tid, [&](unsigned long long key) {
      if ((key & high) == prefix) atomicAdd(&hist[(uint32_t)(key >> shift) & ((1u << width) - 1u)], 1u);
    });
    if (tid < 64) {  // the digit whose bin holds the rank: lane l sums bins l * kPer .., a suffix sum over the lanes
      uint32_t sum = 0u;
      for (int b = 0; b < kPer; ++b) sum += hist[tid * kPer + b];
      uint32_t incl = sum;  // keys in the bins of this lane and of the higher ones
      for (int s = 1; s < 64; s <<= 1) {
        const uint32_t o = (uint32_t)__shfl_down((int)incl, s);
        if (tid + s < 64) incl += o;
      }
      uint32_t above = incl - sum;
      if (above < (uint32_t)want && (uint32_t)want <= incl) {  // exactly one lane (want <= the keys under the prefix)
        for (int b = kPer - 1; b >= 0; --b) {
          const uint32_t c = hist[tid * kPer + b];
          if (above + c >= (uint32_t)want) {
            s_sel[0] = tid * kPer + b;
            s_sel[1] = want - (int)above;
            s_sel[2] = (int)c;
            break;
          }
          above += c;
        }
      }
    }
    __syncthreads();
    prefix |= (unsigned long long)(uint32_t)s_sel[0] << shift;
    want = s_sel[1];
    const bool whole_bin = want == s_sel[2];  // uniform: every key under the prefix is kept -- the cutoff is the prefix
    __syncthreads();                          // (s_sel and the histogram are rewritten by the next digit)
    if (whole_bin) break;
  }
  if (tid == 0) *s_count = 0;
  __syncthreads();
  gft_walk_keys<NT>(g, s_region, tid, [&](unsigned long long key) {
    if (key >= prefix) {
      const int slot = atomicAdd(s_count, 1);
      if (slot < CAND) keys[slot] = key;  // (exactly CAND keys pass)
    }
  });
}

template <int CAND, int NT>
__global__ __launch_bounds__(NT) void gft_select_kernel(const uint2* __restrict__ cand,
                                                              const uint32_t* __restrict__ wcnt, int strip_w, int strips, int nchunks,
                                                              int chunk_rows, int wcap, const uint32_t* __restrict__ mask_bits,
                                                              const uint32_t* __restrict__ mstat, int images_per_maskset,
                                                              int nmask, int rows, int cols, double quality,
                                                              float min_distance, int cell, int max_corners, int cap,
                                                              uint32_t* __restrict__ sorted_g, int sorted_stride,
                                                              float* __restrict__ kp, int32_t* __restrict__ n_out,
                                                              int32_t* __restrict__ status, int32_t* __restrict__ redo,
                                                              int redo_pass, int nimg_total) {
  SOSVO_LATENCY_BOUND_PRIO();
  // Two-pass scheme (redo != nullptr): pass 0 runs the small variant (half the LDS: twice the workgroups per CU of
  // this latency-bound kernel) and hands the few problems that do not fit it -- more candidates than CAND, or a
  // mask bounding box larger than its cell grid -- to pass 1, which runs the full-size variant on those only.
  constexpr int kSelGridCells = (CAND * 8 - 1024 * 4) / 8;  // 2 slots (u32) per cell, 1024 u32 left for the list
  const int p = xcd_problem(nimg_total, nmask);
  if (p < 0) return;  // uniform (padding workgroup)
  if (redo && redo_pass == 1 && redo[p] == 0) return;  // uniform
  __shared__ unsigned long long lds_u64[CAND];
  __shared__ int s_count, s_accepted, s_overflow;
  __shared__ int s_region[NT];  // phase 1: record counts of the regions in flight
  __shared__ int s_sel[3];      // overflow path: digit, rank inside its bin, size of the bin (gft_keep_largest)
  __shared__ unsigned long long s_conf[64];  // phase 3: conflict rows of the round
  __shared__ unsigned long long s_prior;     // phase 3: candidates of the round that conflict with an earlier round's points
  __shared__ int s_ovf;                      // phase 3: accepted points that found both slots of their grid cell taken
  unsigned long long* keys = lds_u64;
  uint32_t* grid = reinterpret_cast<uint32_t*>(lds_u64);  // phase 3: 2 slots per cell, pixel index + 1 (0 = empty)
  uint32_t* acc_list = grid + 2 * kSelGridCells;          // phase 3 fallback: accepted pixel indices (<= 1024)
  const int tid = threadIdx.x;
  const int img = p / nmask, m = p - img * nmask;
  const uint32_t* st = mstat + (size_t)p * 5;                                                              // [0]: max
  const uint32_t* sb = mstat + ((size_t)(img / images_per_maskset) * images_per_maskset * nmask + m) * 5;  // bbox
  uint32_t* sorted = sorted_g + (size_t)p * sorted_stride;
  if (tid == 0) {
    s_count = 0;
    s_accepted = 0;
    s_overflow = 0;
    s_prior = 0ULL;
    s_ovf = 0;
  }
  __syncthreads();
  // ---- phase 1: candidates ------------------------------------------------------------------------------
  const bool any = st[0] != 0u;
  const int bx0 = any ? max(1, (int)(0xFFFFFFFFu - sb[1])) : 0, by0 = any ? max(1, (int)(0xFFFFFFFFu - sb[2])) : 0;
  const int bx1 = any ? min(cols - 2, (int)sb[3] - 1) : -1, by1 = any ? min(rows - 2, (int)sb[4] - 1) : -1;
  const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
  if (any && bw > 0 && bh > 0) {
    const float thr = (float)((double)sosvo_ordered_float(st[0]) * quality);
    const uint32_t* mb = mask_bits + (size_t)(img / images_per_maskset) * rows * cols;
    const int s0 = bx0 / strip_w, s1 = bx1 / strip_w;  // (the strip width of the response kernel that wrote the regions)
    const int c0 = by0 / chunk_rows, c1 = by1 / chunk_rows;
    // The regions (strip, row chunk) that meet the bounding box, NT at a time: every thread fetches ONE region's count (the
    // dependent global loads of a region-by-region walk were most of this phase), then the waves take the regions round-robin,
    // 64 records per step, and claim their key slots with one LDS atomic per wave and step.
    const int ns = s1 - s0 + 1, R = (c1 - c0 + 1) * ns;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    for (int rb = 0; rb < R; rb += NT) {
      if (rb + tid < R) {
        const int rg = rb + tid, c = c0 + rg / ns, sidx = s0 + rg % ns;
        const int have = (int)wcnt[(img * nchunks + c) * strips + sidx];  // the wave numbering of min_eigen_kernel
        if (have > wcap) s_overflow = 1;
        s_region[tid] = min(have, wcap);
      }
      __syncthreads();
      const int rend = min(NT, R - rb);
      for (int rr = wave; rr < rend; rr += NT / 64) {
        const int have = s_region[rr];
        const int rg = rb + rr, c = c0 + rg / ns, sidx = s0 + rg % ns;
        const uint2* region = cand + (size_t)((img * nchunks + c) * strips + sidx) * wcap;
        for (int i0 = 0; i0 < have; i0 += 64) {
          const int i = i0 + lane;
          uint2 r = make_uint2(0u, 0u);
          bool keep = false;
          if (i < have) {
            r = region[i];
            keep = __uint_as_float(r.x) > thr && ((mb[(r.y >> 16) * (uint32_t)cols + (r.y & 0xFFFFu)] >> m) & 1u);
          }
          const unsigned long long km = __ballot(keep);
          if (km) {  // uniform
            const int leader = __ffsll((long long)km) - 1;
            int slot0 = 0;
            if (lane == leader) slot0 = atomicAdd(&s_count, __popcll(km));
            slot0 = __shfl(slot0, leader);
            const int slot = slot0 + __popcll(km & ((1ULL << lane) - 1ULL));
            if (keep && slot < CAND) keys[slot] = ((unsigned long long)sosvo_float_ordered(__uint_as_float(r.x)) << 32) | r.y;
          }
        }
      }
      __syncthreads();  // s_region is rewritten by the next tile
    }
  }
  __syncthreads();
  const int total = s_count;
  if (redo && redo_pass == 0) {  // uniform decision of the whole workgroup
    const int cx0_ = bx0 / cell, cy0_ = by0 / cell;
    const int gw_ = bw > 0 ? bx1 / cell - cx0_ + 1 : 0, gh_ = bh > 0 ? by1 / cell - cy0_ + 1 : 0;
    const bool fits = total <= CAND && (gw_ + 2) * (gh_ + 2) <= kSelGridCells;  // (the bordered grid of phase 3)
    if (tid == 0) redo[p] = fits ? 0 : 1;
    if (!fits) return;
  }
  if (__builtin_expect(total > CAND, 0)) {  // uniform, and rare: the slots above went to whichever waves came first -- gather the CAND largest keys
    const gft_regions g = {cand, wcnt, mask_bits + (size_t)(img / images_per_maskset) * rows * cols, img, m, cols, strips, nchunks, wcap,
                           bx0 / strip_w, by0 / chunk_rows, bx1 / strip_w - bx0 / strip_w + 1,
                           (by1 / chunk_rows - by0 / chunk_rows + 1) * (bx1 / strip_w - bx0 / strip_w + 1),
                           (float)((double)sosvo_ordered_float(st[0]) * quality)};
    gft_keep_largest<CAND, NT>(g, keys, s_region, &s_count, s_sel, tid);
    __syncthreads();
  }
  const int n = min(total, CAND);
  // ---- phase 2: bitonic sort, descending (keys are unique: value, then higher address first) ---------------
  int N = 64;
  while (N < n) N <<= 1;
  for (int i = n + tid; i < N; i += NT) keys[i] = 0ULL;  // padding sorts last
  __syncthreads();
  for (int k = 2, lk = 1; k <= N; k <<= 1, ++lk) {
    // the lk steps of this merge (strides k / 2 ... 1), up to three per pass over the keys (8 keys per thread in registers:
    // a third of the LDS traffic and of the barriers of one step per pass -- the sort is LDS-bandwidth-bound)
    for (int left = lk, j = k >> 1; left > 0;) {
      const int take = left >= 3 ? 3 : left;
      if (take == 3) bitonic_pass<3, NT>(keys, N, k, j, tid);
      else if (take == 2) bitonic_pass<2, NT>(keys, N, k, j, tid);
      else bitonic_pass<1, NT>(keys, N, k, j, tid);
      j >>= take;
      left -= take;
      __syncthreads();
    }
  }
  // candidates leave as packed (y << 16 | x), in order: the low word of the key as it stands
  for (int i = tid; i < n; i += NT) sorted[i] = (uint32_t)keys[i];
  int stt = (total > CAND || s_overflow) ? 1 : 0;
  const int cx0 = bx0 / cell, cy0 = by0 / cell;
  const int gw = bw > 0 ? bx1 / cell - cx0 + 1 : 0, gh = bh > 0 ? by1 / cell - cy0 + 1 : 0;
  const bool use_grid = gw * gh <= kSelGridCells;
  const int limit_list = 1024;
  const float md2 = min_distance * min_distance;
  const bool spaced = min_distance >= 1.0f;
  int limit = cap;
  if (max_corners > 0 && max_corners < limit) limit = max_corners;
  // The usual case runs on integers (gft_igrid: the comparisons are the float ones exactly) with a one-cell border around
  // the grid -- on ALL waves of the workgroup (`fast`, see below) or on the first one.
  const int gwp = gw + 2;
  const bool igrid = spaced && n > 0 && cell <= 2048 && rows <= 32768 && cols <= 32768 && gwp * (gh + 2) <= kSelGridCells;  // uniform
  // (workgroups of eight waves and more -- launches of few problems, where the pass is latency: the C2 batch of 4096 problems
  // keeps the one-wave form, which issues fewer instructions in total: + 0.35 % on the issue-bound step, measured)
  const bool fast = NT > 256 && igrid;
  __syncthreads();  // keys are dead from here on; sorted[] is visible to the whole workgroup
  if (igrid) {
    for (int i = tid; i < gwp * (gh + 2) * 2; i += NT) grid[i] = kGridEmpty;
  } else {
    for (int i = tid; i < (use_grid ? gw * gh * 2 : 0); i += NT) grid[i] = 0u;
  }
  __syncthreads();
  // ---- phase 3: greedy minimum-distance pass ----------------------------------------------------------------
  // 64 candidates per round, in order (every wave holds the round's candidates, one per lane).  (i) Conflicts with points
  // accepted in earlier rounds: cell grid with a border, 9 cells x 2 slots of packed coordinates, no bounds tests, empty
  // slots masked; one cell per work item, the hits OR-ed into s_prior.  (ii) Conflicts INSIDE the round: a 64 x 64 bit
  // matrix, row j = ballot(candidate closer than minDistance to candidate j), one row per work item, left in s_conf.
  // (iii) After the barrier the first wave replays the sequential rule: a survivor of (i) with no EARLIER survivor in its
  // row is accepted whatever happens to the others (decided by all lanes at once); the remaining ones are taken in order on
  // the scalar unit (find-first-bit, two v_readlane, mask tests).  The one-wave form further down recomputes a row per
  // accepted point: a dependent chain of ~10 instructions of a wave that runs alone, 90 ns per point.
  if (fast) {
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const gft_igrid ig(md2, cell, cx0, cy0, gwp);
    int accepted = 0;                                 // uniform over the workgroup
    uint32_t xy_next = lane < n ? sorted[lane] : 0u;  // one coalesced read per 64 candidates, requested a round ahead
    for (int k0 = 0; k0 < n && accepted < limit; k0 += 64) {
      const int kend = min(64, n - k0);
      const bool active = lane < kend;
      const uint32_t xy = xy_next;
      xy_next = k0 + 64 + lane < n ? sorted[k0 + 64 + lane] : 0u;
      const int y = (int)(xy >> 16), x = (int)(xy & 0xFFFFu);
      const int cidx = ig.cell_index(xy, active);  // in the bordered grid
      // (i) + (ii): 9 cell tests and kend matrix rows are 9 + kend work items dealt round-robin over the waves (a lone wave
      // issues an instruction every 5+ cycles and waits for every dependent one: the round is latency, so it is spread)
      constexpr int NWV = NT / 64;
      for (int c9 = wave; c9 < 9; c9 += NWV) {  // uniform per wave
        const unsigned long long hb = __ballot(active && ig.cell_hit(grid, cidx, c9 % 3 - 1, c9 / 3 - 1, xy) != 0u);  // conflict with a point accepted in an earlier round
        if (hb && lane == 0) atomicOr(&s_prior, hb);
      }
      for (int a = wave, novf = min(s_ovf, limit_list); a < novf; a += NWV) {  // (normally empty) uniform per wave
        const unsigned long long hb = __ballot(active && ig.near(xy, acc_list[a]));
        if (hb && lane == 0) atomicOr(&s_prior, hb);
      }
      {
        // rows first + t * NWV, four at a time (independent chains: the scheduler interleaves them); a wave's rows gather in
        // its lanes and leave with one LDS store
        const int first = (wave + NWV - 9 % NWV) % NWV;  // item 9 + j goes to wave (9 + j) % NWV
        uint32_t glo = 0u, ghi = 0u;
        int t = 0;
        for (int jb = first; jb < kend; jb += 4 * NWV, t += 4) {  // uniform per wave
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int j = min(jb + u * NWV, 63);  // (rows beyond kend: computed, never stored)
            const unsigned long long row = __ballot(active && ig.near(xy, (uint32_t)__builtin_amdgcn_readlane((int)xy, j)));
            const bool here = lane == t + u;
            glo = here ? (uint32_t)row : glo;
            ghi = here ? (uint32_t)(row >> 32) : ghi;
          }
        }
        const int jmine = first + lane * NWV;
        if (jmine < kend) s_conf[jmine] = ((unsigned long long)ghi << 32) | glo;
      }
      __syncthreads();
      if (wave == 0) {
        // (iii) a survivor without an EARLIER survivor in its row is accepted whatever happens to the others; the rest are
        // taken in order on the scalar unit: accepted iff no accepted earlier candidate is in their row
        const unsigned long long alive0 = __ballot(active) & ~s_prior;
        const unsigned long long mine = active ? s_conf[lane] : 0ULL;
        const unsigned long long lt = (1ULL << lane) - 1ULL;
        const bool surv = (alive0 >> lane) & 1ULL;
        const unsigned long long fr = __ballot(surv && (mine & alive0 & lt) == 0ULL);
        unsigned long long pending = alive0 & ~fr, acc = fr;
        const int rlo = (int)(uint32_t)mine, rhi = (int)(uint32_t)(mine >> 32);
        while (pending) {
          const int j = __ffsll((long long)pending) - 1;
          pending &= pending - 1ULL;
          const unsigned long long row = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane(rhi, j) << 32) |
                                         (uint32_t)__builtin_amdgcn_readlane(rlo, j);
          if ((row & acc & ((1ULL << j) - 1ULL)) == 0ULL) acc |= 1ULL << j;
        }
        // the sequential pass stops at `limit` points: the first `room` of the accepted ones, in order
        const int room = limit - accepted;
        acc = __ballot(((acc >> lane) & 1ULL) && __popcll(acc & lt) < room);
        if ((acc >> lane) & 1ULL) {
          const int pos = accepted + __popcll(acc & ((1ULL << lane) - 1ULL));
          kp[((size_t)p * cap + pos) * 2] = (float)x;
          kp[((size_t)p * cap + pos) * 2 + 1] = (float)y;
          ig.insert(grid, cidx, xy, &s_ovf, acc_list, limit_list);
        }
        if (lane == 0) {
          s_accepted = accepted + __popcll(acc);
          s_prior = 0ULL;  // (read above by this wave only; the others add to it after the barrier)
        }
      }
      __syncthreads();
      accepted = s_accepted;
    }
    if (s_ovf > limit_list) stt |= 2;
  } else if (NT <= 256 && igrid) {
    // One-wave form on the integer grid (workgroups of four waves: launches of more than 1024 problems).  The control flow is
    // that of the float form below -- which candidate is accepted when is the sequential rule, replayed point by point --
    // with the spread form's arithmetic: nine unconditional cell reads, one v_readlane and one packed distance per accepted
    // point, no division, no bounds test, no conversion.
    if (tid < 64) {
      const int lane = tid;
      const gft_igrid ig(md2, cell, cx0, cy0, gwp);
      int accepted = 0;
      uint32_t xy_next = lane < n ? sorted[lane] : 0u;  // one coalesced read per 64 candidates, requested a round ahead
      for (int k0 = 0; k0 < n && accepted < limit; k0 += 64) {
        const int kend = min(64, n - k0);
        const bool active = lane < kend;
        const uint32_t xy = xy_next;
        xy_next = k0 + 64 + lane < n ? sorted[k0 + 64 + lane] : 0u;
        const int cidx = ig.cell_index(xy, active);
        uint32_t prior = 0u;  // conflict with a point accepted in an earlier round
#pragma unroll 1
        for (int dyc = -1; dyc <= 1; ++dyc)  // a row of three cells at a time: six slots in flight, not eighteen (registers)
#pragma unroll
          for (int dxc = -1; dxc <= 1; ++dxc) prior |= ig.cell_hit(grid, cidx, dxc, dyc, xy);
        for (int a = 0, novf = min(s_ovf, limit_list); a < novf; ++a) prior |= (uint32_t)ig.near(xy, acc_list[a]);  // (normally none)
        unsigned long long alive = __ballot(active && prior == 0u);
        unsigned long long acc = 0ULL;
        int room = limit - accepted;
        while (alive && room > 0) {
          const int j = __ffsll((long long)alive) - 1;
          alive &= alive - 1ULL;
          acc |= 1ULL << j;
          room--;
          alive &= ~__ballot(ig.near(xy, (uint32_t)__builtin_amdgcn_readlane((int)xy, j)));
        }
        if ((acc >> lane) & 1ULL) {
          const int pos = accepted + __popcll(acc & ((1ULL << lane) - 1ULL));
          kp[((size_t)p * cap + pos) * 2] = (float)(xy & 0xFFFFu);
          kp[((size_t)p * cap + pos) * 2 + 1] = (float)(xy >> 16);
          ig.insert(grid, cidx, xy, &s_ovf, acc_list, limit_list);
        }
        accepted += __popcll(acc);
      }
      if (lane == 0) s_accepted = accepted;
    }
  } else
  if (tid < 64) {  // one-wave form (float distances; the accepted points in a list when the grid does not fit)
    const int lane = tid;
    if (!use_grid && limit_list < limit) {
      limit = limit_list;
      stt |= 2;
    }
    int accepted = 0;
    uint32_t xy_next = lane < n ? sorted[lane] : 0u;  // one coalesced read per 64 candidates, requested a round ahead
    for (int k0 = 0; k0 < n && accepted < limit; k0 += 64) {
      const int kend = min(64, n - k0);
      const bool active = lane < kend;
      const uint32_t xy = xy_next;
      xy_next = k0 + 64 + lane < n ? sorted[k0 + 64 + lane] : 0u;
      const int y = (int)(xy >> 16), x = (int)(xy & 0xFFFFu);
      bool prior = false;  // conflict with a point accepted in an earlier round
      if (active && spaced) {
        if (use_grid) {
          const int xc = x / cell - cx0, yc = y / cell - cy0;
#pragma unroll
          for (int c9 = 0; c9 < 9; ++c9) {
            const int xx = xc + (c9 % 3) - 1, yy = yc + (c9 / 3) - 1;
            if (xx < 0 || xx >= gw || yy < 0 || yy >= gh) continue;
            const uint2 q2 = *reinterpret_cast<const uint2*>(&grid[(yy * gw + xx) * 2]);
#pragma unroll
            for (int slot = 0; slot < 2; ++slot) {
              const uint32_t q = slot ? q2.y : q2.x;
              if (q) {
                const float dx = (float)(x - (int)((q - 1u) & 0xFFFFu)), dy = (float)(y - (int)((q - 1u) >> 16));
                prior = prior || (dx * dx + dy * dy < md2);
              }
            }
          }
          for (int a = 0, novf = min(s_ovf, limit_list); a < novf; ++a) {  // third points of their cells (normally none)
            const uint32_t q = acc_list[a];
            const float dx = (float)(x - (int)(q & 0xFFFFu)), dy = (float)(y - (int)(q >> 16));
            prior = prior || (dx * dx + dy * dy < md2);
          }
        } else {
          for (int a = 0; a < accepted; ++a) {
            const uint32_t q = acc_list[a];
            const float dx = (float)(x - (int)(q & 0xFFFFu)), dy = (float)(y - (int)(q >> 16));
            prior = prior || (dx * dx + dy * dy < md2);
          }
        }
      }
      unsigned long long alive = __ballot(active && !prior);
      unsigned long long acc = 0ULL;
      int room = limit - accepted;
      while (alive && room > 0) {
        const int j = __ffsll((long long)alive) - 1;
        alive &= alive - 1ULL;
        acc |= 1ULL << j;
        room--;
        if (spaced) {
          const int xj = __builtin_amdgcn_readlane(x, j), yj = __builtin_amdgcn_readlane(y, j);
          const float dx = (float)(x - xj), dy = (float)(y - yj);
          alive &= ~__ballot(dx * dx + dy * dy < md2);
        }
      }
      if ((acc >> lane) & 1ULL) {
        const int pos = accepted + __popcll(acc & ((1ULL << lane) - 1ULL));
        kp[((size_t)p * cap + pos) * 2] = (float)x;
        kp[((size_t)p * cap + pos) * 2 + 1] = (float)y;
        if (spaced) {
          if (use_grid) {
            uint32_t* c = &grid[((y / cell - cy0) * gw + (x / cell - cx0)) * 2];
            if (atomicCAS(&c[0], 0u, xy + 1u) != 0u && atomicCAS(&c[1], 0u, xy + 1u) != 0u) {  // third point of a cell
              const int o = atomicAdd(&s_ovf, 1);
              if (o < limit_list) acc_list[o] = xy;  // (an overflow is reported once, after the loop, from s_ovf)
            }
          } else {
            acc_list[pos] = xy;
          }
        }
      }
      accepted += __popcll(acc);
    }
    if (lane == 0) s_accepted = accepted;
  }
  __syncthreads();
  if (tid == 0) {
    if (s_ovf > limit_list) stt |= 2;  // the overflowing lane is not tid 0 in general: decide from the shared counter
    n_out[p] = min(s_accepted, cap);
    if (status) status[p] = stt;
  }
}

// ---- K6a: 7x7 Gaussian, 8.8 fixed point ------------------------------------------------------------------
// Same rolling layout as min_eigen_kernel: a wave owns a 64-column strip (58 output columns) and walks down a
// chunk of rows; the six horizontal neighbours come from neighbouring lanes (mirrored lanes at the image
// border = reflect-101), the seven rows of horizontal sums live in a register ring.
__global__ __launch_bounds__(kThreads) void gauss7_kernel(const uint8_t* __restrict__ gray, long long img_stride, int nimg,
                                                          int rows, int cols, int strips, int nchunks, int chunk_rows,
                                                          uint8_t* __restrict__ out, long long out_stride,
                                                          const int32_t* __restrict__ row_range, int imgs_per_range) {
  SOSVO_STREAMING_PRIO();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * kThreads + threadIdx.x) >> 6));  // in an SGPR: per-image bases become scalar
  if (wave >= nimg * strips * nchunks) return;  // wave-uniform
  const int img = wave / (strips * nchunks);
  const int rem = wave - img * strips * nchunks;
  const int chunk = rem / strips, strip = rem - chunk * strips;
  const int xb = strip * kEigStripW - kEigHalo;
  const int xc = xb + lane;
  const int xs = clampi(xc, 0, cols - 1);
  int src[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) src[k] = clampi(refl101(xs + k - 3, cols) - xb, 0, 63);
  const bool out_lane = lane >= kEigHalo && lane < 64 - kEigHalo && xc < cols;
  int ys = chunk * chunk_rows, ye = min(rows, ys + chunk_rows);
  if (row_range) {  // only the rows a reader of the blurred image can reach (see sosvo_describe_orb_rows); wave-uniform
    const int v = img / imgs_per_range;
    ys = max(ys, row_range[2 * v]);
    ye = min(ye, row_range[2 * v + 1]);
    if (ys >= ye) return;
  }
  const uint8_t* g = gray + (size_t)img * img_stride;  // (img_stride = rows * cols for a dense batch; a pyramid level of
  uint8_t* o = out + (size_t)img * out_stride;        //  the ORB detector sits at a fixed offset of a larger per-image block)
  // seven-deep ring of horizontal sums indexed by (row mod 7): the row loop is unrolled seven times by a fold
  uint32_t h[7] = {0, 0, 0, 0, 0, 0, 0};
  const bool edge_strip = xb < 3 || xb + 64 > cols - 3;  // wave-uniform: some lane's x-3 .. x+3 are mirrored columns
  const int t_first = ys - 3, t_last = ye + 2;
  // gray rows in two half-batches into the ring slots just emptied, three to six steps ahead of their use (round 4, as
  // orb_level_pass_kernel: one row ahead does not cover a load that misses the L2)
  int c_pre[7];
  auto request = [&](int t0, int k0, int k1) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < 7; ++k)
      if (k >= k0 && k < k1) c_pre[k] = (int)g[(uint32_t)(refl101(min(t0 + k, t_last), rows) * cols) + (uint32_t)xs];
  };
  request(t_first, 0, 7);
  auto step = [&](auto phase_tag, auto edge_tag, const int t) __attribute__((always_inline)) {
    constexpr int P = decltype(phase_tag)::value;
    constexpr bool EDGE = decltype(edge_tag)::value;
    if (t > t_last) return;  // uniform
    const int c = c_pre[P];  // gray row t
    int l1, l2, l3, r1, r2, r3;
    if (EDGE) {
      l3 = __shfl(c, src[0]); l2 = __shfl(c, src[1]); l1 = __shfl(c, src[2]);
      r1 = __shfl(c, src[4]); r2 = __shfl(c, src[5]); r3 = __shfl(c, src[6]);
    } else {
      l1 = lane_from_left(c); l2 = lane_from_left(l1); l3 = lane_from_left(l2);
      r1 = lane_from_right(c); r2 = lane_from_right(r1); r3 = lane_from_right(r2);
    }
    // (24-bit multiplies -- every operand is below 2^18, every sum below 2^24 -- so that each tap is ONE v_mad_u32_u24
    // instead of a 32-bit multiply plus an add)
    h[P] = vmad24(18u, (uint32_t)(l3 + r3), vmad24(34u, (uint32_t)(l2 + r2), vmad24(49u, (uint32_t)(l1 + r1), 54u * (uint32_t)c)));
    const int y = t - 3;
    if (y < ys) return;  // uniform
    // rows y-3 .. y+3 = t-6 .. t live in slots P+1 .. P+7 (mod 7)
    const uint32_t vsum = vmad24(18u, h[(P + 1) % 7] + h[P], vmad24(34u, h[(P + 2) % 7] + h[(P + 6) % 7],
                                vmad24(49u, h[(P + 3) % 7] + h[(P + 5) % 7], 54u * h[(P + 4) % 7])));
    if (out_lane) o[(uint32_t)(y * cols) + (uint32_t)xc] = (uint8_t)((vsum + 32768u) >> 16);
  };
  auto run = [&](auto edge_tag) __attribute__((always_inline)) {
    for (int t = t_first; t <= t_last; t += 7) {
      step(std::integral_constant<int, 0>{}, edge_tag, t);
      step(std::integral_constant<int, 1>{}, edge_tag, t + 1);
      step(std::integral_constant<int, 2>{}, edge_tag, t + 2);
      step(std::integral_constant<int, 3>{}, edge_tag, t + 3);
      request(t + 7, 0, 4);
      step(std::integral_constant<int, 4>{}, edge_tag, t + 4);
      step(std::integral_constant<int, 5>{}, edge_tag, t + 5);
      step(std::integral_constant<int, 6>{}, edge_tag, t + 6);
      request(t + 7, 4, 7);
    }
  };
  if (edge_strip) run(std::true_type{}); else run(std::false_type{});
}

// ---- K6a, four columns per lane -------------------------------------------------------------------------------
// The same rolling walk with a lane holding four adjacent gray bytes of a row as one dword C (layout, load offsets and the
// border rule: rolling_layout.h): a wave covers 256 columns and owns 250 outputs.  L and R are the neighbouring lanes' dwords
// (two lane moves per row for four pixels instead of six for one); the horizontal sum of pixel j of the lane is two
// v_dot4_u32_u8, over the bytes j-3 .. j with the weights (18, 34, 49, 54) and over j+1 .. j+4 with (49, 34, 18, 0), the byte
// windows cut out of (L, C) and (C, R) by v_alignbyte_b32 -- the windows of j = 3 are C and R themselves.  Integer arithmetic
// below 2^24: the value is gauss7_kernel's whatever the order.  The vertical pass is per pixel as there; the rounding
// constant rides in the first multiply-add, and the four output bytes leave as one dword where all four columns are outputs
// inside the image, in smaller stores otherwise.
// At the image border (EDGE instantiation) one v_perm_b32 per row turns the lane's load -- taken at an offset clamped into
// the row -- into its four virtual columns, mirrored ones included; L and R then come from the neighbours as in the interior.
// Lanes 0 / 63 receive L = 0 / R = 0: byte 3 of lane 0 does not read L, and byte 0 of lane 63 reads R under the weight 0.
__global__ __launch_bounds__(kThreads) void gauss7_wide_kernel(const uint8_t* __restrict__ gray, long long img_stride, int nimg,
                                                               int rows, int cols, int strips, int nchunks, int chunk_rows,
                                                               uint8_t* __restrict__ out, long long out_stride,
                                                               const int32_t* __restrict__ row_range, int imgs_per_range) {
  SOSVO_STREAMING_PRIO();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * kThreads + threadIdx.x) >> 6));
  if (wave >= nimg * strips * nchunks) return;  // wave-uniform
  const int img = wave / (strips * nchunks);
  const int rem = wave - img * strips * nchunks;
  const int chunk = rem / strips, strip = rem - chunk * strips;
  const sosvo_blur_wide_lane lay = sosvo_blur_wide_layout(cols, strip, lane);
  const int x0 = strip * SOSVO_BLUR_WIDE_STRIP_W - 3 + 4 * lane;  // the lane's first column: a store happens only where it is inside the image
  int ys = chunk * chunk_rows, ye = min(rows, ys + chunk_rows);
  if (row_range) {  // wave-uniform, as in gauss7_kernel
    const int v = img / imgs_per_range;
    ys = max(ys, row_range[2 * v]);
    ye = min(ye, row_range[2 * v + 1]);
    if (ys >= ye) return;
  }
  const uint8_t* g = gray + (size_t)img * img_stride;
  uint8_t* o = out + (size_t)img * out_stride;
  // The lane's outputs are a run of nb adjacent bytes from byte jb on (lay.own): all four leave as a dword, otherwise two of
  // them as a 16-bit store and / or the last one as a byte (lanes 0 and 63 own one column each; so may the lane that holds the
  // image's last column).  Stores touch owned columns only: x0 + jb >= 0 wherever a store is enabled.
  const int jb = lay.own ? __builtin_ctz(lay.own) : 0, nb = __builtin_popcount(lay.own);
  const bool st_dword = nb == 4, st_short = nb == 2 || nb == 3, st_byte = nb == 1 || nb == 3;
  const uint32_t st_x = (uint32_t)(x0 + jb), st_shift = 8u * (uint32_t)jb;
  const uint32_t st_xb = (uint32_t)(x0 + jb + nb - 1), st_shiftb = 8u * (uint32_t)(st_byte ? jb + nb - 1 : 0);
  const uint32_t ld_x = (uint32_t)lay.off;
  uint32_t h[7][4];
#pragma unroll
  for (int k = 0; k < 7; ++k) h[k][0] = h[k][1] = h[k][2] = h[k][3] = 0u;
  const bool edge_strip = sosvo_blur_wide_edge_strip(cols, strip) != 0;  // wave-uniform
  const int t_first = ys - 3, t_last = ye + 2;
  const uint32_t w_lo = 0x36312212u, w_hi = 0x00122231u;  // byte weights (18, 34, 49, 54) and (49, 34, 18, 0)
  uint32_t c_pre[7];
  auto request = [&](int t0, int k0, int k1) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < 7; ++k)
      if (k >= k0 && k < k1)
        c_pre[k] = *reinterpret_cast<const u32_unaligned*>(g + ((uint32_t)(refl101(min(t0 + k, t_last), rows) * cols) + ld_x));
  };
  request(t_first, 0, 7);
  auto step = [&](auto phase_tag, auto edge_tag, const int t) __attribute__((always_inline)) {
    constexpr int P = decltype(phase_tag)::value;
    constexpr bool EDGE = decltype(edge_tag)::value;
    if (t > t_last) return;  // uniform
    uint32_t c = c_pre[P];   // gray row t
    if (EDGE) c = __builtin_amdgcn_perm(c, c, lay.sel);
    const uint32_t l = (uint32_t)lane_from_left((int)c), r = (uint32_t)lane_from_right((int)c);
#pragma unroll
    for (int j = 0; j < 3; ++j)
      h[P][j] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(c, l, j + 1), w_lo,
                                       __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(r, c, j + 1), w_hi, 0u, false), false);
    h[P][3] = __builtin_amdgcn_udot4(c, w_lo, __builtin_amdgcn_udot4(r, w_hi, 0u, false), false);
    const int y = t - 3;
    if (y < ys) return;  // uniform
    // rows y-3 .. y+3 = t-6 .. t live in slots P+1 .. P+7 (mod 7); s = vertical sum + 32768, the output byte is its bits 16 .. 23
    uint32_t s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      s[j] = vmad24(18u, h[(P + 1) % 7][j] + h[P][j], vmad24(34u, h[(P + 2) % 7][j] + h[(P + 6) % 7][j],
                    vmad24(49u, h[(P + 3) % 7][j] + h[(P + 5) % 7][j], vmad24(54u, h[(P + 4) % 7][j], 32768u))));
    const uint32_t p01 = __builtin_amdgcn_perm(s[1], s[0], 0x0C0C0602u), p23 = __builtin_amdgcn_perm(s[3], s[2], 0x0C0C0602u);
    const uint32_t pk = __builtin_amdgcn_perm(p23, p01, 0x05040100u);
    const uint32_t oy = (uint32_t)(y * cols);
    if (st_dword) *reinterpret_cast<u32_unaligned*>(o + (oy + st_x)) = pk;
    if (st_short) *reinterpret_cast<u16_unaligned*>(o + (oy + st_x)) = (uint16_t)(pk >> st_shift);
    if (st_byte) o[oy + st_xb] = (uint8_t)(pk >> st_shiftb);
  };
  auto run = [&](auto edge_tag) __attribute__((always_inline)) {
    for (int t = t_first; t <= t_last; t += 7) {
      step(std::integral_constant<int, 0>{}, edge_tag, t);
      step(std::integral_constant<int, 1>{}, edge_tag, t + 1);
      step(std::integral_constant<int, 2>{}, edge_tag, t + 2);
      step(std::integral_constant<int, 3>{}, edge_tag, t + 3);
      request(t + 7, 0, 4);
      step(std::integral_constant<int, 4>{}, edge_tag, t + 4);
      step(std::integral_constant<int, 5>{}, edge_tag, t + 5);
      step(std::integral_constant<int, 6>{}, edge_tag, t + 6);
      request(t + 7, 4, 7);
    }
  };
  if (edge_strip) run(std::true_type{}); else run(std::false_type{});
}

// ---- K6b: border rule + descriptors ---------------------------------------------------------------------
constexpr int kPatchMaxR = 23, kPatchRows = 48, kPatchStride = 64;
constexpr int kDescRegionBytesGft = 24 * 1024;

// The rotated BRIEF pattern depends on (pattern, cos_a, sin_a) only: one workgroup per CALL writes it to the call's
// workspace, every problem's workgroup reads it.  pt[t] is test t's two points in pixels, rounded to nearest, each as
// dy << 16 | (dx & 0xFFFF) (|dx|, |dy| <= 181: int8 coordinates times sqrt 2); R = max(|dx|, |dy|) over all of them; poff
// the points' byte offsets in a per-keypoint LDS patch (origin R before the keypoint, rows 4 * pstride bytes apart, pstride a
// function of R), zero when R is beyond the patches.  (Per call and in stream order, never kept across calls: the caller
// owns `pattern` and may rewrite it in place.)
__host__ __device__ __forceinline__ int orb_patch_stride_dw(int R) { return ((2 * R + 1 + 3) >> 2) | 1; }  // row pitch in dwords, odd
struct orb_pattern_table {
  int2 pt[256];
  int R, pad;
  uint16_t poff[512];
};
__global__ __launch_bounds__(256) void orb_pattern_table_kernel(const int8_t* __restrict__ pattern, float cos_a, float sin_a,
                                                                orb_pattern_table* __restrict__ tab) {
  __shared__ int s_R;
  const int t = threadIdx.x;
  if (t == 0) s_R = 0;
  __syncthreads();
  int d[4];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const float px = (float)pattern[4 * t + 2 * e], py = (float)pattern[4 * t + 2 * e + 1];
    const float xr = (px * cos_a) - (py * sin_a), yr = (px * sin_a) + (py * cos_a);
    d[2 * e] = __float2int_rn(xr);
    d[2 * e + 1] = __float2int_rn(yr);
  }
  tab->pt[t] = make_int2((int)(((uint32_t)d[1] << 16) | ((uint32_t)d[0] & 0xFFFFu)), (int)(((uint32_t)d[3] << 16) | ((uint32_t)d[2] & 0xFFFFu)));
  atomicMax(&s_R, max(max(abs(d[0]), abs(d[1])), max(abs(d[2]), abs(d[3]))));
  __syncthreads();
  const int R = s_R;
  if (t == 0) tab->R = R;
  const int pitch = R <= kPatchMaxR ? 4 * orb_patch_stride_dw(R) : 0;
  tab->poff[2 * t] = (uint16_t)(R <= kPatchMaxR ? (d[1] + R) * pitch + (d[0] + R) : 0);
  tab->poff[2 * t + 1] = (uint16_t)(R <= kPatchMaxR ? (d[3] + R) * pitch + (d[2] + R) : 0);
}

// (NT threads: a problem's keypoints are shared by NT / 64 waves, one keypoint per wave and step -- 256 for the C2 batch of
// 4096 problems, 512 when a launch has few problems, 1024 for the whole-image problems of up to 4096 keypoints)
template <int NT>
__global__ __launch_bounds__(NT) void orb_describe_kernel(const uint8_t* __restrict__ blurred, int rows, int cols,
                                                                int nmask, int cap, float* __restrict__ kp,
                                                                int32_t* __restrict__ n_io, const orb_pattern_table* __restrict__ ptab, int edge,
                                                                uint8_t* __restrict__ desc, int nimg_total,
                                                                const int32_t* __restrict__ row_range, int imgs_per_range) {
  SOSVO_LATENCY_BOUND_PRIO();
  extern __shared__ float lds_kp[];  // [cap][2] compacted keypoints
  // one LDS area, two uses (NT = 256, the batch of (image, mask) problems): the REGION of the blurred image under all of the
  // problem's keypoints (below), or the waves' per-keypoint patches; the larger workgroups keep the patches only
  constexpr int kPatchWords = (NT / 64) * (kPatchRows * kPatchStride / 4);
  constexpr int kRegionWords = NT == 256 ? kDescRegionBytesGft / 4 : 0;
  __shared__ uint32_t patch_area[kPatchWords > kRegionWords ? kPatchWords : kRegionWords];
  __shared__ int wave_off[NT / 64 + 1];
  __shared__ int s_running;
  __shared__ int s_bb[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int p = xcd_problem(nimg_total, nmask);
  if (p < 0) return;  // uniform (padding workgroup)
  const int img = p / nmask;
  const int n = min(n_io[p], cap);
  if (tid == 0) s_running = 0;
  __syncthreads();
  const int R = ptab->R;  // uniform
  // this lane's four tests (lane, 64 + lane, 128 + lane, 192 + lane) as offsets from a keypoint in an array whose rows lie
  // `pitch` apart: multiply-adds on the table's (dx, dy)
  // (the table pointer goes through an empty asm in the path that calls this: the eight loads then stay in that path, next to
  // their use, and are not hoisted to the top of the kernel to be carried across the compaction and the staging)
  auto lane_offsets = [&](int pitch, int* a, int* b) __attribute__((always_inline)) {
    const int2* tp = ptab->pt;
    asm volatile("" : "+s"(tp));
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int2 d = tp[64 * r + lane];
      a[r] = (d.x >> 16) * pitch + (int)(short)d.x;
      b[r] = (d.y >> 16) * pitch + (int)(short)d.y;
    }
  };
  // A descriptor's four ballots to its 32 bytes: lane 0 holds the eight halves (eight moves of scalars) and stores them as
  // two 16-byte pieces at a 32-bit offset from the problem's first row, a scalar.  (`desc` is 8-byte aligned, hence the type.)
  struct __attribute__((packed, aligned(8))) desc_half { uint32_t w[4]; };
  uint8_t* const desc_p = desc + (size_t)p * cap * 32;
  auto store_desc = [&](int j, const unsigned long long* bal) __attribute__((always_inline)) {
    if (lane == 0) {
      desc_half* d = reinterpret_cast<desc_half*>(desc_p + ((uint32_t)j << 5));
      d[0] = desc_half{{(uint32_t)bal[0], (uint32_t)(bal[0] >> 32), (uint32_t)bal[1], (uint32_t)(bal[1] >> 32)}};
      d[1] = desc_half{{(uint32_t)bal[2], (uint32_t)(bal[2] >> 32), (uint32_t)bal[3], (uint32_t)(bal[3] >> 32)}};
    }
  };
  // Patch path: the (2R+1)^2 neighbourhood of a keypoint goes through LDS, fetched as unaligned dwords -- a few
  // row segments per lane instead of 512 scattered byte loads.  Patch rows are `pstride` dwords apart with
  // pstride ODD, so the rows spread over all 32 banks (a 64-byte row pitch would leave half of them unused and
  // turn the scattered byte reads of the tests into 4-6-way conflicts).  The dword overrun past a patch row
  // (<= 3 bytes) stays inside the image as long as the border rule keeps R + 1 px.
  const bool patch_ok = R <= kPatchMaxR && edge >= R + 1;
  const int PR = 2 * R + 1;
  // With a row range only the blurred rows [rr_lo, rr_hi) exist, and those within 3 rows of an inner end were blurred
  // from gray rows outside the range: a keypoint whose patch rows leave the trustworthy part is REMOVED, like one too
  // close to the image border (callers that derive the range from the keypoints' masks never lose one this way).
  int y_first = 0, y_last = rows - 1;
  if (row_range) {
    const int v = img / imgs_per_range;
    const int rr_lo = row_range[2 * v], rr_hi = row_range[2 * v + 1];
    y_first = (rr_lo <= 0 ? 0 : rr_lo + 3) + R;
    y_last = (rr_hi >= rows ? rows : rr_hi - 3) - 1 - R;
  }
  const int pdw = (PR + 3) >> 2;      // dwords per patch row
  const int pstride = orb_patch_stride_dw(R);  // row pitch in dwords: pdw | 1
  for (int i0 = 0; i0 < n; i0 += NT) {
    const int i = i0 + tid;
    float x = 0.f, y = 0.f;
    bool keep = false;
    if (i < n) {
      x = kp[((size_t)p * cap + i) * 2];
      y = kp[((size_t)p * cap + i) * 2 + 1];
      keep = x >= (float)edge && x < (float)(cols - edge) && y >= (float)edge && y < (float)(rows - edge);
      const int yi = __float2int_rn(y);
      keep = keep && yi >= y_first && yi <= y_last;
    }
    const int pos = sosvo_block_compact_pos<NT / 64>(keep, wave_off, &s_running, tid);
    if (keep) {
      lds_kp[2 * pos] = x;
      lds_kp[2 * pos + 1] = y;
    }
  }
  __syncthreads();
  const int m = s_running;
  for (int i = tid; i < 2 * m; i += NT) kp[(size_t)p * cap * 2 + i] = lds_kp[i];
  if (tid == 0) n_io[p] = m;
  const uint8_t* im = blurred + (size_t)img * rows * cols;
  // ---- the usual case of the (image, mask) batch: every keypoint from ONE staged region (round 4) -------------------------
  // The ~165 keypoints of an azimuthal mask lie so close together that their (2R + 1)^2 patches cover the same pixels about
  // nine times over, and fetched per keypoint they are 390 scattered dwords each through the texture addresser (0.8 G dword
  // accesses per 256 frame pairs: more than any other kernel of the step).  The bounding box of the problem's keypoints grown
  // by R goes to LDS once (coalesced dword loads, ~20 KB for a 120-column mask of a 146-row panorama); the tests read it.
  if constexpr (NT == 256) {
    if (patch_ok && m > 0) {  // uniform
      if (tid < 4) s_bb[tid] = tid < 2 ? 0x7FFFFFFF : -1;
      __syncthreads();
      for (int i = tid; i < m; i += NT) {
        const int cx = __float2int_rn(lds_kp[2 * i]), cy = __float2int_rn(lds_kp[2 * i + 1]);
        atomicMin(&s_bb[0], cx);
        atomicMin(&s_bb[1], cy);
        atomicMax(&s_bb[2], cx);
        atomicMax(&s_bb[3], cy);
      }
      __syncthreads();
      const int rx0 = s_bb[0] - R, ry0 = s_bb[1] - R, rw = s_bb[2] - s_bb[0] + PR, rh = s_bb[3] - s_bb[1] + PR;
      const int ldw = (rw + 3) >> 2, pitch_dw = ldw | 1, pitch_b = 4 * pitch_dw;
      if (pitch_b * rh <= kDescRegionBytesGft) {  // uniform
        {  // eight requests in flight per thread, the position advanced without a division
          const int step_r = NT / ldw, step_k = NT - step_r * ldw;
          int ry = tid / ldw, k = tid - ry * ldw;
          const uint8_t* org = im + (size_t)ry0 * cols + rx0;
          while (__any(ry < rh)) {
            uint32_t v[8];
            int dst[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              dst[u] = ry < rh ? ry * pitch_dw + k : -1;
              v[u] = *reinterpret_cast<const u32_unaligned*>(org + (uint32_t)(min(ry, rh - 1) * cols + 4 * k));
              k += step_k;
              ry += step_r;
              if (k >= ldw) {
                k -= ldw;
                ++ry;
              }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
              if (dst[u] >= 0) patch_area[dst[u]] = v[u];
          }
        }
        // Every keypoint's origin inside the region, once: the float pair of keypoint i is read by this thread only (kp has
        // its copy already), so the origin takes the place of its x.  __float2int_rn of the same floats: the same integers
        // as the bounding box saw.
        int* lds_org = reinterpret_cast<int*>(lds_kp);
        for (int i = tid; i < m; i += NT) {
          const int cx = __float2int_rn(lds_kp[2 * i]), cy = __float2int_rn(lds_kp[2 * i + 1]);
          lds_org[2 * i] = (cy - ry0) * pitch_b + (cx - rx0);
        }
        // this lane's eight test points as LDS addresses of the region's origin (tests lane, 64 + lane, 128 + lane,
        // 192 + lane): the region's base is folded in here, so that a test address in the loop is ONE addition
        typedef __attribute__((address_space(3))) const uint8_t lds_u8;
        int ra[4], rb[4];
        lane_offsets(pitch_b, ra, rb);
        const int region_base = (int)(uintptr_t)(lds_u8*)reinterpret_cast<const uint8_t*>(patch_area);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          ra[r] += region_base;
          rb[r] += region_base;
          asm volatile("" : "+v"(ra[r]), "+v"(rb[r]));
        }
        __syncthreads();
        const int wid_s = __builtin_amdgcn_readfirstlane(wid);
        for (int j = wid_s; j < m; j += NT / 64) {
          const int org = lds_org[2 * j];  // (the same value in every lane)
          unsigned long long bal[4];
#pragma unroll
          for (int r = 0; r < 4; ++r)
            bal[r] = __ballot(*(lds_u8*)(uintptr_t)(uint32_t)(org + ra[r]) < *(lds_u8*)(uintptr_t)(uint32_t)(org + rb[r]));
          store_desc(j, bal);
        }
        return;
      }
      __syncthreads();  // (the per-keypoint patches below reuse the area)
    }
  }
  if (patch_ok) {
    uint32_t* patch32 = patch_area + wid * (kPatchRows * kPatchStride / 4);
    const uint8_t* patch = reinterpret_cast<const uint8_t*>(patch32);
    // 8 lanes (dwords) per patch row and 8 rows per round while a row fits 32 bytes, else 16 lanes x 4 rows.  Lanes
    // past the row's last dword / rows past the patch repeat the last one (same value to the same LDS word), so the
    // loads and the LDS writes are unconditional: no exec-mask juggling around a dozen memory instructions.
    const int lsh = pdw <= 8 ? 3 : 4;
    const int prow = lane >> lsh, pk = min(lane & ((1 << lsh) - 1), pdw - 1);
    const int rpr = 64 >> lsh, nit = (PR + rpr - 1) / rpr;  // rows per round, rounds (<= kPatchRows / 4)
    uint32_t reg[kPatchRows / 4];
    int goff[kPatchRows / 4], lidx[kPatchRows / 4];  // per round: image byte offset / LDS word of this lane's dword
#pragma unroll
    for (int it = 0; it < kPatchRows / 4; ++it) {
      const int r = min(rpr * it + prow, PR - 1);
      goff[it] = r * cols;
      lidx[it] = r * pstride + pk;
    }
    auto issue = [&](int j) {
      const uint8_t* base =
          im + ((size_t)__float2int_rn(lds_kp[2 * j + 1]) - R) * cols + (__float2int_rn(lds_kp[2 * j]) - R) + 4 * pk;
#pragma unroll
      for (int it = 0; it < kPatchRows / 4; ++it)
        if (it < nit) reg[it] = *reinterpret_cast<const u32_unaligned*>(base + goff[it]);  // uniform test
    };
    // this lane's eight patch offsets (tests lane, 64 + lane, 128 + lane, 192 + lane) never change: registers
    int pa[4], pb[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      pa[r] = ptab->poff[2 * (64 * r + lane)];
      pb[r] = ptab->poff[2 * (64 * r + lane) + 1];
    }
    int j = wid;
    if (j < m) issue(j);
    for (; j < m; j += NT / 64) {
#pragma unroll
      for (int it = 0; it < kPatchRows / 4; ++it)
        if (it < nit) patch32[lidx[it]] = reg[it];
      if (j + NT / 64 < m) issue(j + NT / 64);  // next keypoint's rows fly while this one is tested
      unsigned long long bal[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) bal[r] = __ballot(patch[pa[r]] < patch[pb[r]]);
      store_desc(j, bal);
    }
    return;
  }
  int ga[4], gb[4];
  lane_offsets(cols, ga, gb);
  for (int j = wid; j < m; j += NT / 64) {
    const uint8_t* c = im + (size_t)__float2int_rn(lds_kp[2 * j + 1]) * cols + __float2int_rn(lds_kp[2 * j]);
    unsigned long long bal[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) bal[r] = __ballot(c[ga[r]] < c[gb[r]]);
    store_desc(j, bal);
  }
}

// Row chunks of the rolling kernels: enough waves to fill 1024 SIMDs several times over, chunks of >= 24 rows
// (6 halo rows each).
static void rolling_chunks(int nimg, int rows, int strips, int* nchunks, int* chunk_rows) {
  int nc = cdiv(16384, nimg * strips);
  if (nc > rows / 24) nc = rows / 24;
  if (nc < 1) nc = 1;
  *chunk_rows = cdiv(rows, nc);
  *nchunks = cdiv(rows, *chunk_rows);
}

// Row chunks of the four-columns-per-lane form.  A wave of it carries the work of four of the one-column form's, so the
// 16 384-wave target above would cut the bench's batch (1024 images per part, 6 strips of 1440 columns) into three chunks
// and pay 6 halo rows in each: + 12 % of rows for nothing.  The target here is the number of waves the chip needs, not a
// multiple of it: 6 per SIMD in one pass, 6 144.  A batch whose (image, strip) pairs reach that runs unchunked; a smaller
// one (a window of a sequence, a single frame) is cut into cdiv(6144, pairs) chunks of at least 24 rows, as before.
static void rolling_chunks_wide(int nimg, int rows, int strips, int* nchunks, int* chunk_rows) {
  int nc = cdiv(6144, nimg * strips);
  if (nc > rows / 24) nc = rows / 24;
  if (nc < 1) nc = 1;
  *chunk_rows = cdiv(rows, nc);
  *nchunks = cdiv(rows, *chunk_rows);
}

}  // namespace

// 7x7 sigma-2 blur (8.8 fixed point) of nimg images that lie img_stride bytes apart (shared with the ORB pyramid levels).
// Four columns per lane (gauss7_wide_kernel) from SOSVO_BLUR_WIDE_MIN_COLS columns on, unless SOSVO_HINT_ROLLING_NARROW
// asks for the one-column form; the bytes are the same, and so is the profile label.
static int32_t launch_gauss7_rows(sosvo_ctx* ctx, const uint8_t* in, long long in_stride, int nimg, int rows, int cols,
                                  uint8_t* out, long long out_stride, const int32_t* row_range, int imgs_per_range) {
  int nchunks, chunk_rows;
  if (cols >= SOSVO_BLUR_WIDE_MIN_COLS && !ctx->hint_rolling_narrow) {
    const int strips = sosvo_blur_wide_strips(cols);
    rolling_chunks_wide(nimg, rows, strips, &nchunks, &chunk_rows);
    {
      SOSVO_PROFILE(ctx, "gauss7_kernel");
      hipLaunchKernelGGL(gauss7_wide_kernel, dim3(cdiv(nimg * strips * nchunks, kThreads / 64)), dim3(kThreads), 0, ctx->stream, in,
                         in_stride, nimg, rows, cols, strips, nchunks, chunk_rows, out, out_stride, row_range, imgs_per_range);
    }
    SOSVO_LAUNCH_CHECK(ctx);
    return SOSVO_OK;
  }
  const int strips = cdiv(cols, kEigStripW);
  rolling_chunks(nimg, rows, strips, &nchunks, &chunk_rows);
  SOSVO_LAUNCH(ctx, gauss7_kernel, dim3(cdiv(nimg * strips * nchunks, kThreads / 64)), dim3(kThreads), 0, ctx->stream, in,
               in_stride, nimg, rows, cols, strips, nchunks, chunk_rows, out, out_stride, row_range, imgs_per_range);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}
int32_t sosvo_launch_gauss7_rows(sosvo_ctx* ctx, const uint8_t* in, long long in_stride, int nimg, int rows, int cols,
                                 uint8_t* out, long long out_stride, const int32_t* row_range, int imgs_per_range) {
  return launch_gauss7_rows(ctx, in, in_stride, nimg, rows, cols, out, out_stride, row_range, imgs_per_range);
}
int32_t sosvo_launch_gauss7_to(sosvo_ctx* ctx, const uint8_t* in, long long in_stride, int nimg, int rows, int cols,
                               uint8_t* out, long long out_stride) {
  return launch_gauss7_rows(ctx, in, in_stride, nimg, rows, cols, out, out_stride, nullptr, 1);
}
int32_t sosvo_launch_gauss7(sosvo_ctx* ctx, const uint8_t* in, long long img_stride, int nimg, int rows, int cols,
                            uint8_t* out) {
  return sosvo_launch_gauss7_to(ctx, in, img_stride, nimg, rows, cols, out, img_stride);
}

// Geometry of one corner-response launch.  Two columns per lane
// (min_eigen_wide_kernel, strips of 61 columns, a wave per PAIR of strips) from kEigWideMinCols columns on, unless
// SOSVO_HINT_ROLLING_NARROW asks for the one-column form (strips of 58, a wave per strip); regions are numbered
// (img * nchunks + chunk) * strips + strip in both, and gft_select_kernel gets the strip width that was used.
struct gft_plan {
  bool wide;
  int strip_w, strips, nchunks, chunk_rows, wcap, waves;
  size_t n_regions;
};
static gft_plan gft_plan_make(const sosvo_ctx* ctx, int nimg, int rows, int cols, int nmask) {
  gft_plan g;
  g.wide = cols >= kEigWideMinCols && !ctx->hint_rolling_narrow;
  g.strip_w = g.wide ? kEigWideStripW : kEigStripW;
  g.strips = cdiv(cols, g.strip_w);
  if (g.wide)
    rolling_chunks_wide(nimg, rows, cdiv(g.strips, 2), &g.nchunks, &g.chunk_rows);
  else
    rolling_chunks(nimg, rows, g.strips, &g.nchunks, &g.chunk_rows);
  g.waves = nimg * g.nchunks * (g.wide ? cdiv(g.strips, 2) : g.strips);
  // candidate records (8 bytes: response, pixel): a region per (strip, row chunk) with room for EVERY pixel of it -- 3x3
  // maxima of distinct values fill at most a quarter of it, but an exactly periodic texture gives a plateau of equal
  // positive responses on which every pixel is a candidate, and goodFeaturesToTrack handles that; only what is written
  // costs traffic
  g.wcap = (g.chunk_rows * g.strip_w + 63) & ~63;
  g.n_regions = (size_t)nimg * g.strips * g.nchunks;
  return g;
}
// The scratch of a plan: the response kernel's outputs, then (sosvo_detect_gft, sorted_stride > 0) what the selection adds
struct gft_bufs {
  uint2* cand;
  uint32_t *wcnt, *mstat, *sorted;
  int32_t* redo;
};
static gft_bufs gft_carve(Carver& cv, const gft_plan& g, size_t P, int sorted_stride) {
  gft_bufs b;
  b.cand = cv.take<uint2>(g.n_regions * g.wcap);
  b.wcnt = cv.take<uint32_t>(g.n_regions);
  b.mstat = cv.take<uint32_t>(P * 5);
  b.sorted = cv.take<uint32_t>(P * sorted_stride);
  b.redo = cv.take<int32_t>(sorted_stride ? P : 0);
  return b;
}
// mstat cleared, mask bounding boxes, the response kernel: candidate records, their counts and the per-mask maxima
static int32_t gft_launch_response(sosvo_ctx* ctx, const gft_plan& g, const gft_bufs& b, const uint8_t* gray, const uint32_t* mask_bits,
                                   int nimg, int images_per_maskset, int rows, int cols, int nmask) {
  uint2* cand = b.cand;
  uint32_t *wcnt = b.wcnt, *mstat = b.mstat;
  SOSVO_HIP(ctx, hipMemsetAsync(mstat, 0, sizeof(uint32_t) * (size_t)nimg * nmask * 5, ctx->stream));
  const int nsets = cdiv(nimg, images_per_maskset);
  SOSVO_LAUNCH(ctx, mask_bbox_kernel, dim3(rows, nsets), dim3(kThreads), 0, ctx->stream, mask_bits, images_per_maskset, rows,
               cols, nmask, mstat);
  SOSVO_LAUNCH_CHECK(ctx);
  if (g.wide) {
    SOSVO_PROFILE(ctx, "min_eigen_kernel");
    hipLaunchKernelGGL(min_eigen_wide_kernel, dim3(cdiv(g.waves, kThreads / 64)), dim3(kThreads), 0, ctx->stream, gray, mask_bits,
                       nimg, images_per_maskset, rows, cols, nmask, g.strips, g.nchunks, g.chunk_rows, g.wcap, cand, wcnt, mstat);
  } else {
    SOSVO_LAUNCH(ctx, min_eigen_kernel, dim3(cdiv(g.waves, kThreads / 64)), dim3(kThreads), 0, ctx->stream, gray, mask_bits, nimg,
                 images_per_maskset, rows, cols, nmask, g.strips, g.nchunks, g.chunk_rows, g.wcap, cand, wcnt, mstat);
  }
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

extern "C" {

int32_t sosvo_detect_gft_candidates(sosvo_ctx* ctx, const uint8_t* gray, const uint32_t* mask_bits, int32_t nimg,
                                    int32_t images_per_maskset, int32_t rows, int32_t cols, int32_t nmask, int32_t* geometry,
                                    uint32_t* cand_out, uint32_t* wcnt_out, uint32_t* mstat_out) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, geometry, "null pointer");
  SOSVO_REQUIRE(ctx, nimg >= 1 && nimg <= 65535 && images_per_maskset > 0, "nimg out of range");
  SOSVO_REQUIRE(ctx, rows >= 3 && cols >= 3 && rows * (int64_t)cols < (1 << 28), "image sizes out of range");
  SOSVO_REQUIRE(ctx, rows <= 65535 && cols <= 65535, "image sizes out of range (the candidates are packed as y << 16 | x)");
  SOSVO_REQUIRE(ctx, nmask >= 1 && nmask <= kMaxMasks, "nmask out of range (1..32)");
  const gft_plan g = gft_plan_make(ctx, nimg, rows, cols, nmask);
  SOSVO_REQUIRE(ctx, g.n_regions * (size_t)g.wcap < ((size_t)1 << 31), "too many candidate slots for this entry point");
  geometry[0] = g.strip_w;
  geometry[1] = g.strips;
  geometry[2] = g.nchunks;
  geometry[3] = g.chunk_rows;
  geometry[4] = g.wcap;
  geometry[5] = (int32_t)g.n_regions;
  if (!cand_out && !wcnt_out && !mstat_out) return SOSVO_OK;  // the sizes only
  SOSVO_REQUIRE(ctx, gray && mask_bits && cand_out && wcnt_out && mstat_out, "null pointer");
  gft_bufs b;
  int32_t rc = sosvo_ws_carve(ctx, [&](Carver& cv) { b = gft_carve(cv, g, (size_t)nimg * nmask, 0); });
  if (rc != SOSVO_OK) return rc;
  rc = gft_launch_response(ctx, g, b, gray, mask_bits, nimg, images_per_maskset, rows, cols, nmask);
  if (rc != SOSVO_OK) return rc;
  SOSVO_HIP(ctx, hipMemcpyAsync(cand_out, b.cand, sizeof(uint2) * g.n_regions * g.wcap, hipMemcpyDeviceToDevice, ctx->stream));
  SOSVO_HIP(ctx, hipMemcpyAsync(wcnt_out, b.wcnt, sizeof(uint32_t) * g.n_regions, hipMemcpyDeviceToDevice, ctx->stream));
  SOSVO_HIP(ctx, hipMemcpyAsync(mstat_out, b.mstat, sizeof(uint32_t) * (size_t)nimg * nmask * 5, hipMemcpyDeviceToDevice, ctx->stream));
  return SOSVO_OK;
}

int32_t sosvo_detect_gft(sosvo_ctx* ctx, const uint8_t* gray, const uint32_t* mask_bits, int32_t nimg,
                         int32_t images_per_maskset, int32_t rows, int32_t cols, int32_t nmask, double quality,
                         double min_distance, int32_t max_corners, int32_t cap, float* kp, int32_t* n,
                         int32_t* status) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, gray && mask_bits && kp && n, "null pointer");
  SOSVO_REQUIRE(ctx, nimg >= 0 && nimg <= 65535 && images_per_maskset > 0, "nimg out of range");
  SOSVO_REQUIRE(ctx, rows >= 3 && cols >= 3 && rows * (int64_t)cols < (1 << 28), "image sizes out of range");
  SOSVO_REQUIRE(ctx, rows <= 65535 && cols <= 65535, "image sizes out of range (the candidates are packed as y << 16 | x)");
  SOSVO_REQUIRE(ctx, nmask >= 1 && nmask <= kMaxMasks, "nmask out of range (1..32)");
  // quality >= 1 is legal as in cv2.goodFeaturesToTrack: the threshold quality * max is then >= every response (the
  // candidate records hold the POSITIVE local maxima only), so no corner passes `v > thr` and every count comes back 0
  SOSVO_REQUIRE(ctx, cap > 0 && cap <= 4096 && quality > 0 && min_distance >= 0, "bad detector parameters (quality > 0)");
  if (nimg == 0) return SOSVO_OK;
  const size_t P = (size_t)nimg * nmask;
  const gft_plan g = gft_plan_make(ctx, nimg, rows, cols, nmask);
  const int strip_w = g.strip_w, strips = g.strips, nchunks = g.nchunks, chunk_rows = g.chunk_rows, wcap = g.wcap;
  const bool large = cap > 1024;  // whole-image masks (RGB-D frames): 16384 candidates, 15872 grid cells
  const int sorted_stride = large ? kCandCapLarge : kCandCap;
  gft_bufs b;
  int32_t rc = sosvo_ws_carve(ctx, [&](Carver& cv) { b = gft_carve(cv, g, P, sorted_stride); });
  if (rc != SOSVO_OK) return rc;
  uint2* cand = b.cand;
  uint32_t *wcnt = b.wcnt, *mstat = b.mstat, *sorted_g = b.sorted;
  rc = gft_launch_response(ctx, g, b, gray, mask_bits, nimg, images_per_maskset, rows, cols, nmask);
  if (rc != SOSVO_OK) return rc;
  const int cell = min_distance >= 1 ? (int)lrint(min_distance) : 1;
  int32_t* redo = b.redo;
  if (large) {
    SOSVO_PROFILE(ctx, "gft_select_kernel");
    hipLaunchKernelGGL((gft_select_kernel<kCandCapLarge, 1024>), dim3(xcd_grid(nimg, nmask)), dim3(1024), 0, ctx->stream, cand, wcnt,
                       strip_w, strips, nchunks, chunk_rows, wcap, mask_bits, mstat, images_per_maskset, nmask, rows, cols, quality, (float)min_distance, cell,
                       max_corners, cap, sorted_g, sorted_stride, kp, n, status, nullptr, 0, nimg);
  } else {
    // Few problems (a window of a sequence, a handful of large frames): eight waves per workgroup share the rounds of the
    // greedy pass and the sort; many problems (the C2 batch: 4096 per launch): four, so that twice as many are resident.
    SOSVO_PROFILE(ctx, "gft_select_kernel");
    auto launch = [&](auto small, auto full, int nt) {
      hipLaunchKernelGGL(small, dim3(xcd_grid(nimg, nmask)), dim3(nt), 0, ctx->stream, cand, wcnt, strip_w, strips, nchunks, chunk_rows, wcap,
                         mask_bits, mstat, images_per_maskset, nmask, rows, cols, quality, (float)min_distance, cell, max_corners, cap,
                         sorted_g, sorted_stride, kp, n, status, redo, 0, nimg);
      hipLaunchKernelGGL(full, dim3(xcd_grid(nimg, nmask)), dim3(nt), 0, ctx->stream, cand, wcnt, strip_w, strips, nchunks, chunk_rows, wcap,
                         mask_bits, mstat, images_per_maskset, nmask, rows, cols, quality, (float)min_distance, cell, max_corners, cap,
                         sorted_g, sorted_stride, kp, n, status, redo, 1, nimg);
    };
    if (P <= 1024)
      launch(gft_select_kernel<kCandCapSmall, 512>, gft_select_kernel<kCandCap, 512>, 512);
    else
      launch(gft_select_kernel<kCandCapSmall, kThreads>, gft_select_kernel<kCandCap, kThreads>, kThreads);
  }
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

int32_t sosvo_gauss7(sosvo_ctx* ctx, const uint8_t* gray, int32_t nimg, int32_t rows, int32_t cols, int64_t img_stride,
                     uint8_t* out, int64_t out_stride, const int32_t* row_range) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, gray && out, "null pointer");
  SOSVO_REQUIRE(ctx, nimg >= 0 && nimg <= 65535, "nimg out of range");
  SOSVO_REQUIRE(ctx, rows >= 1 && cols >= 1 && rows * (int64_t)cols < (1 << 28), "image sizes out of range");
  SOSVO_REQUIRE(ctx, img_stride >= rows * (int64_t)cols && out_stride >= rows * (int64_t)cols, "a stride is shorter than an image");
  SOSVO_REQUIRE(ctx, row_range == nullptr || nimg % 2 == 0, "row_range needs the two views' images (nimg even, view-major)");
  if (nimg == 0) return SOSVO_OK;
  return launch_gauss7_rows(ctx, gray, img_stride, nimg, rows, cols, out, out_stride, row_range, nimg > 1 ? nimg / 2 : 1);
}

int32_t sosvo_describe_orb(sosvo_ctx* ctx, const uint8_t* gray, int32_t nimg, int32_t rows, int32_t cols,
                           int32_t nmask, int32_t cap, float* kp, int32_t* n, float cos_a, float sin_a,
                           const int8_t* pattern, int32_t edge, uint8_t* desc) {
  return sosvo_describe_orb_rows(ctx, gray, nimg, rows, cols, nmask, cap, kp, n, cos_a, sin_a, pattern, edge, nullptr, desc);
}

int32_t sosvo_describe_orb_rows(sosvo_ctx* ctx, const uint8_t* gray, int32_t nimg, int32_t rows, int32_t cols,
                                int32_t nmask, int32_t cap, float* kp, int32_t* n, float cos_a, float sin_a,
                                const int8_t* pattern, int32_t edge, const int32_t* row_range, uint8_t* desc) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, row_range == nullptr || nimg % 2 == 0, "row_range needs the two views' images (nimg even, view-major)");
  SOSVO_REQUIRE(ctx, gray && kp && n && pattern && desc, "null pointer");
  SOSVO_REQUIRE(ctx, nimg >= 0 && nimg <= 65535 && nmask >= 1, "nimg / nmask out of range");
  SOSVO_REQUIRE(ctx, rows >= 1 && cols >= 1 && rows * (int64_t)cols < (1 << 28), "image sizes out of range");
  SOSVO_REQUIRE(ctx, cap > 0 && cap <= 4096, "cap out of range");
  SOSVO_REQUIRE(ctx, edge >= 19, "edge must cover the rotated 31x31 patch (>= 19)");
  SOSVO_REQUIRE(ctx, ((uintptr_t)desc & 7) == 0, "desc must be 8-byte aligned");
  if (nimg == 0) return SOSVO_OK;
  uint8_t* blurred;
  orb_pattern_table* ptab;  // the rotated pattern of THIS call, next to the blurred images
  int32_t rc = sosvo_ws_carve(ctx, [&](Carver& cv) {
    blurred = cv.take<uint8_t>((size_t)nimg * rows * cols);
    ptab = cv.take<orb_pattern_table>(1);
  });
  if (rc != SOSVO_OK) return rc;
  SOSVO_LAUNCH(ctx, orb_pattern_table_kernel, dim3(1), dim3(256), 0, ctx->stream, pattern, cos_a, sin_a, ptab);
  SOSVO_LAUNCH_CHECK(ctx);
  rc = launch_gauss7_rows(ctx, gray, (long long)rows * cols, nimg, rows, cols, blurred, (long long)rows * cols, row_range,
                          nimg > 1 ? nimg / 2 : 1);
  if (rc != SOSVO_OK) return rc;
  const size_t lds_kp_bytes = (size_t)cap * 2 * sizeof(float);
  const int irange = nimg > 1 ? nimg / 2 : 1;
  SOSVO_PROFILE(ctx, "orb_describe_kernel");
  auto launch = [&](auto kernel, int nt) {
    hipLaunchKernelGGL(kernel, dim3(xcd_grid(nimg, nmask)), dim3(nt), lds_kp_bytes, ctx->stream, blurred, rows, cols, nmask, cap, kp,
                       n, ptab, edge, desc, nimg, row_range, irange);
  };
  if (cap > 1024)
    launch(orb_describe_kernel<1024>, 1024);
  else if ((size_t)nimg * nmask <= 1024)
    launch(orb_describe_kernel<512>, 512);
  else
    launch(orb_describe_kernel<kThreads>, kThreads);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

}  // extern "C"
