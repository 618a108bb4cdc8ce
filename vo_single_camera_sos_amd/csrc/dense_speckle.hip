// Speckle filter of the dense disparity map: connected-component labelling of d16 [n, rows, cols]
// under the relation include/sosvo.h states for sosvo_dense_speckle (tests/refspeckle.py is the same text in numpy), and the
// removal of every component of at most max_size pixels.  What cv2.filterSpeckles' flood fill computes, as union-find.
//
// One forest per frame in parent [n, rows, cols] u32, indices relative to the frame.  Three facts carry everything:
//   1. parent[x] <= x at every instant: the init kernel writes a run's first pixel (or x); the merge kernel hangs a root
//      below a smaller root and a node below a smaller node of its tree; the label kernel stores a root.  So a find walks
//      strictly downward and ends after at most x + 1 loads, whatever it reads and whenever: no loop here can spin.
//   2. Trees only grow: a root is hung below a smaller root by compare-and-swap on its own entry, and every other store
//      replaces a link by one to a smaller node of the same tree.  So whatever a walk reads, however out of date (an L1,
//      another compute die's L2), lies in x's tree from then on: it costs steps and never a wrong answer, and the decisive read
//      is the one inside the compare-and-swap, which is the true one.
//   3. The root of a finished tree is its smallest index, so labels and sizes depend on no order of arrival.
// Four launches: init (row runs by ballot, sizes zeroed), merge (vertical joins that the pair to the left does not already
// imply, the panorama's seam), label (label = root in place, one atomicAdd on its size per label and wave), apply.  The
// atomics are ordinary vector atomics on global memory.
#include "common.h"

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;  // the label of an invalid pixel

// Relaxed atomics of wavefront scope: plain loads and stores through the L1 that the compiler may neither hoist out of a
// loop nor tear.  (Agent scope, which goes past the L1 and, for a store, drops the line from the L2, was measured: the merge
// kernel took 3.7 times as long at n = 64.  What the L1 serves out of date costs a step, fact 2.)
__device__ __forceinline__ uint32_t load_parent(const uint32_t* parent, uint32_t x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

__device__ __forceinline__ void store_parent(uint32_t* parent, uint32_t x, uint32_t v) {
  __hip_atomic_store(parent + x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// The node at which the walk from x stops.  Bounded by fact 1: x decreases with every step.
__device__ __forceinline__ uint32_t find_root(const uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = load_parent(parent, x);
    if (p >= x) return x;
    x = p;
  }
}

// The same walk, and every node it passes is hung below its grandparent (path halving), so that a chain met once is half
// as long for whoever comes next.  What is stored was read two links above x: smaller than x and in its tree (facts 1, 2).
__device__ __forceinline__ uint32_t find_root_halving(uint32_t* parent, uint32_t x) {
  uint32_t p = load_parent(parent, x);
  if (p >= x) return x;
  for (;;) {
    const uint32_t g = load_parent(parent, p);
    if (g >= p) return p;
    store_parent(parent, x, g);
    x = p;
    p = g;
  }
}

// Joins the trees of a and b: the larger root is hung below the smaller by compare-and-swap on its OWN entry, so that a
// tree is never split (the halving above relies on it; atomicMin on the entry could replace a link that another lane had
// made and split the tree until that lane's next round, which is why it is not used).  A round that does
// not end replaces a by what the swap found in its entry, which is smaller than a, and the walks never increase either
// node: at most a + b rounds.
__device__ __forceinline__ void merge(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = find_root_halving(parent, a);
    b = find_root_halving(parent, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    const uint32_t old = atomicCAS(parent + a, a, b);
    if (old == a) return;  // a was a root and now hangs below b
    a = old;               // (a had stopped being a root: go on from its parent)
  }
}

__device__ __forceinline__ bool joined(int a, int b, int max_diff) { return a >= 0 && b >= 0 && abs(a - b) <= max_diff; }

// One block per row of one frame, 256 columns per round: parent = the first pixel of the pixel's run of joined horizontal
// neighbours (the highest break at or below the lane in the wave's ballot, else the last break of an earlier wave or round).
__global__ __launch_bounds__(256) void speckle_init_kernel(const int16_t* __restrict__ d16, int rows, int cols, int max_diff,
                                                           uint32_t* __restrict__ parent, uint32_t* __restrict__ size) {
  __shared__ int last_break[2][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = blockIdx.x;
  const size_t row0 = ((size_t)blockIdx.y * rows + r) * cols;
  const uint32_t rel0 = (uint32_t)r * cols;
  int carry = 0;  // the last break before this round's columns (column 0 is one)
  for (int base = 0, round = 0; base < cols; base += 256, ++round) {
    const int c = base + threadIdx.x;
    const bool in = c < cols;
    const int d = in ? d16[row0 + c] : -1;
    const int dl = in && c > 0 ? d16[row0 + c - 1] : -1;
    const bool brk = !joined(d, dl, max_diff);  // (an invalid pixel breaks too; its own parent is kNone)
    const uint64_t breaks = __ballot(brk);
    if (lane == 0) last_break[round & 1][wave] = breaks ? base + wave * 64 + 63 - __builtin_clzll(breaks) : -1;
    __syncthreads();  // (the other buffer is written next round, after every wave has passed this barrier)
    const uint64_t below = breaks & (~0ULL >> (63 - lane));
    int start = below ? base + wave * 64 + 63 - __builtin_clzll(below) : -1;
    int before = carry, last = carry;  // the nearest break before this wave's columns / up to the end of this round
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int lb = last_break[round & 1][w];
      if (lb >= 0) {
        if (w < wave) before = lb;
        last = lb;
      }
    }
    if (start < 0) start = before;
    if (in) {
      parent[row0 + c] = d >= 0 ? rel0 + (uint32_t)start : kNone;
      size[row0 + c] = 0;
    }
    carry = last;
  }
}

// One lane per pixel: the join with the pixel above, unless the column to the left already makes it (both horizontal
// pairs and the left vertical pair joined: the same two runs), and in column 0 with `cyclic` the join across the seam.
__global__ __launch_bounds__(256) void speckle_merge_kernel(const int16_t* __restrict__ d16, int rows, int cols, int max_diff, int cyclic,
                                                            uint32_t* __restrict__ parent) {
  const uint32_t frame_pixels = (uint32_t)rows * cols, p = blockIdx.x * 256u + threadIdx.x;
  if (p >= frame_pixels) return;
  const size_t f0 = (size_t)blockIdx.y * frame_pixels;
  const int16_t* d = d16 + f0;
  uint32_t* par = parent + f0;
  const int v = d[p];
  if (v < 0) return;
  const int r = (int)(p / (uint32_t)cols), c = (int)(p - (uint32_t)r * cols);
  if (r > 0) {
    const int up = d[p - cols];
    if (joined(v, up, max_diff)) {
      bool implied = false;
      if (c > 0) {
        const int left = d[p - 1], upleft = d[p - cols - 1];
        implied = joined(v, left, max_diff) && joined(up, upleft, max_diff) && joined(left, upleft, max_diff);
      }
      if (!implied) merge(par, p, p - cols);
    }
  }
  if (cyclic && c == 0 && cols > 1 && joined(v, d[p + cols - 1], max_diff)) merge(par, p, p + cols - 1);
}

// label = root, stored in place (a walker that meets a stored root only arrives sooner; the roots themselves do not change),
// and size[label] += 1 per valid pixel with one atomicAdd per label and wave: the lanes that hold the label of the first lane
// still waiting are counted by a ballot and leave (at most 64 rounds, one per label in the wave; a large component, whose
// one address every wave adds to, costs one add per wave).
__global__ __launch_bounds__(256) void speckle_label_kernel(int rows, int cols, uint32_t* __restrict__ parent, uint32_t* __restrict__ size,
                                                            uint32_t* __restrict__ labels_out) {
  const uint32_t frame_pixels = (uint32_t)rows * cols, p = blockIdx.x * 256u + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const size_t f0 = (size_t)blockIdx.y * frame_pixels;
  uint32_t l = kNone;
  if (p < frame_pixels) {
    uint32_t* par = parent + f0;
    l = load_parent(par, p);
    if (l != kNone && l < p) {
      l = find_root(par, l);
      store_parent(par, p, l);
    }
    if (labels_out) labels_out[f0 + p] = l;
  }
  uint64_t waiting = __ballot(l != kNone);
  while (waiting) {  // (uniform: every round clears at least the first waiting lane)
    const int first = __builtin_ctzll(waiting);
    const uint32_t lf = (uint32_t)__shfl((int)l, first);
    const uint64_t same = __ballot(l == lf);
    if (lane == first) atomicAdd(size + f0 + lf, (uint32_t)__popcll(same));
    waiting &= ~same;
  }
}

__global__ __launch_bounds__(256) void speckle_apply_kernel(const int16_t* d16, const uint32_t* __restrict__ label,
                                                            const uint32_t* __restrict__ size, int rows, int cols, uint32_t max_size,
                                                            int16_t* d16_out) {  // (d16_out may be d16: a lane reads its own pixel first)
  const uint32_t frame_pixels = (uint32_t)rows * cols, p = blockIdx.x * 256u + threadIdx.x;
  if (p >= frame_pixels) return;
  const size_t f0 = (size_t)blockIdx.y * frame_pixels;
  const int16_t v = d16[f0 + p];
  const uint32_t l = label[f0 + p];
  d16_out[f0 + p] = (l != kNone && size[f0 + l] <= max_size) ? (int16_t)-1 : v;
}

}  // namespace

extern "C" int32_t sosvo_dense_speckle(sosvo_ctx* ctx, const int16_t* d16, int32_t n, int32_t rows, int32_t cols, int32_t max_size,
                                       int32_t max_diff, int32_t flags, int16_t* d16_out, uint32_t* labels_out) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, d16 && d16_out, "null pointer");
  SOSVO_REQUIRE_DENSE_SIZE(ctx, rows, cols);
  SOSVO_REQUIRE_DENSE_N(ctx, n);
  SOSVO_REQUIRE(ctx, max_size >= 0, "max_size is negative");
  SOSVO_REQUIRE(ctx, max_diff >= 0 && max_diff <= 32767, "max_diff out of range (0..32767)");
  SOSVO_REQUIRE_DENSE_FLAGS(ctx, flags);
  const size_t frame_pixels = (size_t)rows * cols, total = (size_t)n * frame_pixels;
  uint32_t *parent, *size;
  const int32_t rc = sosvo_ws_carve(ctx, [&](Carver& cv) {
    parent = cv.take<uint32_t>(total);
    size = cv.take<uint32_t>(total);
  });
  if (rc != SOSVO_OK) return rc;
  const dim3 per_pixel((unsigned)((frame_pixels + 255) / 256), n);
  SOSVO_LAUNCH(ctx, speckle_init_kernel, dim3(rows, n), dim3(256), 0, ctx->stream, d16, rows, cols, max_diff, parent, size);
  SOSVO_LAUNCH_CHECK(ctx);
  SOSVO_LAUNCH(ctx, speckle_merge_kernel, per_pixel, dim3(256), 0, ctx->stream, d16, rows, cols, max_diff,
               (flags & SOSVO_DENSE_CYCLIC_COLUMNS) != 0 ? 1 : 0, parent);
  SOSVO_LAUNCH_CHECK(ctx);
  SOSVO_LAUNCH(ctx, speckle_label_kernel, per_pixel, dim3(256), 0, ctx->stream, rows, cols, parent, size, labels_out);
  SOSVO_LAUNCH_CHECK(ctx);
  SOSVO_LAUNCH(ctx, speckle_apply_kernel, per_pixel, dim3(256), 0, ctx->stream, d16, parent, size, rows, cols, (uint32_t)max_size,
               d16_out);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}
