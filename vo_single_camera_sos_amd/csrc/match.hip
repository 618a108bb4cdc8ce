// K7 -- brute-force Hamming matching and the stable sort of matches by distance.
//
// Reference call sites: cv2.BFMatcher(NORM_HAMMING).match / knnMatch at
// omnistereo/camera_models.py:442 / :420 and sorted(matches, key=distance) at :444.
//
// Mapping to CDNA4: the 1-NN / 2-NN search is an exact integer contraction on the MATRIX cores
// (hamming = |q| + |t| - 2 q.t on descriptors unpacked to one byte per bit, v_mfma_i32_32x32x32_i8; see
// match_hamming_mfma_kernel) -- the step around it is VALU-issue bound, the matrix pipe was idle.  The result is
// carried as the packed key (distance << 20 | train index): an unsigned min over keys is exactly "smallest
// distance, first train index wins", so partial results of train-range splits merge with
// one atomicMin and stay bit-identical to a sequential scan.  Round 1-2 ran this stage on the VALU (one query per
// lane in 8 VGPRs, train tile in LDS read as broadcasts, 8 x (v_xor + v_bcnt) per pair: 18 VALU wave-instructions per
// 64 pairs against ~2.5 now); the radius search (not on the VO path) still does.
#include <math.h>

#include <algorithm>

#include "common.h"

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ uint32_t hamming256(const uint4& a0, const uint4& a1, const uint4& b0,
                                               const uint4& b1) {
  uint32_t d = __popc(a0.x ^ b0.x);
  d += __popc(a0.y ^ b0.y);
  d += __popc(a0.z ^ b0.z);
  d += __popc(a0.w ^ b0.w);
  d += __popc(a1.x ^ b1.x);
  d += __popc(a1.y ^ b1.y);
  d += __popc(a1.z ^ b1.z);
  d += __popc(a1.w ^ b1.w);
  return d;
}

// ---- K7 on the matrix pipe ------------------------------------------------------------------------------
// hamming(q, t) = |q| + |t| - 2 q.t on 0/1 vectors: the pair distances of a (32 trains x 32 queries) tile are ONE exact
// integer contraction over K = 256, i.e. eight v_mfma_i32_32x32x32_i8 on descriptors unpacked to one byte per bit.  The
// step around this kernel is VALU-issue bound and MFMA issues beside VALU, so the 8 x (xor + popcount) per pair of the
// round-2 kernel (18 VALU wave-instructions per 64 pairs) shrink to HALF an instruction per pair-element, and the
// contraction itself runs on the otherwise idle matrix cores:
//   operand values: a train bit is the byte 16, a query bit the byte -16, so the contraction yields -256 q.t = (-2 q.t) << 7;
//     the accumulator is not cleared but STARTS at base7[row] = |t| << 7 | row-in-tile (the 16 accumulator registers of a
//     lane are 4 x ds_read_b128 of that LDS table), so after the eight MFMAs every accumulator register already IS the
//     tile-local partial key ((|t| - 2 q.t) << 7) + row -- ordered like the packed key (|q| is constant per lane): the
//     epilogue is one v_min3_i32 per TWO pair-elements.  Once per 128-train tile the winner is widened to
//     ((|t| - 2 q.t) << 20) + train index; |q| << 20 is added at the very end.  Rows past the train count start at 2^24.
//   unpacking: any permutation of the 256 bit positions applied to both sides keeps q.t, so the cheapest one is used:
//     dword w of a descriptor -> K-block w; lane half h (= lane / 32) takes the bits {s + 4 h + 8 b}: operand dword s =
//     ((h ? x : x << 4) >> s) & 0x10101010, byte b.  A operands (trains): unpacked once per workgroup into an LDS tile (row
//     pitch 272 B: conflict-free ds_read_b128 across the 16-lane groups); B operands (queries): 32 VGPRs per 32-query tile.
//   accumulator r of lane l is (train row 8 (r / 4) + 4 (l / 32) + r % 4, query column l % 32).
// Two entry kernels, one body: match_hamming_mfma_kernel<QT, K> (the 1-NN / 2-NN search over every train) and
// match_hamming_gated_mfma_kernel<QT, DV> (guided matching: the 1-NN search over the trains that pass sv_pixel_gate,
// geom_core.h, against the query: key(i) = min over admissible j of (hamming << 20 | j)) are match_hamming_mfma_body with
// GATED off and on.  The contraction, the operand layout and the base7 preload exist once; the gated form adds:
//   the train tile also stages the positions, as DOUBLES in structure-of-arrays order (tu[128], tv[128]): the four rows of
//     an accumulator group are 32 consecutive bytes per coordinate, two ds_read_b128; the conversion float -> double is
//     paid once per train and tile, not per pair;
//   a lane keeps its query's position resident as doubles;
//   the epilogue evaluates the gate on doubles -- fabs(u_t - u_q) <= max_du and v_t - v_q >= min_dv, literally
//     sv_pixel_gate's expressions, so equal to the assemble kernels' for every finite float32 input (a float32 subtraction
//     would round a difference just above max_du onto it) -- and replaces a failing element by kMmaInvalid with one select
//     before the min chain.  None of this depends on the accumulators, so it is scheduled beside the MFMAs.
//   DV = false drops the v side (the frame-to-frame form pays for du only).  A disabled du side is max_du = +inf (the
//     difference of two finite float32 is finite in double), decided by the host.
//   reversed problems (p >= n_forward) negate both v coordinates while staging: (-v_t) - (-v_q) is v_q - v_t exactly, and
//     fabs(u_t - u_q) is symmetric, so the gate of the swapped roles costs nothing per pair.
//   the cap: a winner whose distance exceeds max_distance is stored as SOSVO_KEY_NONE.  With a train-range split each
//     partial winner is capped before its atomicMin: the overall winner has the smallest admissible distance, so it is
//     stored iff it is within the cap, and no partial that loses to it matters.
// RATIO (match_hamming_ratio_mfma_kernel<QT, GATED, DV>, sosvo_match_hamming_ratio): Lowe's distinctiveness rule on the
// device.  The body tracks the runner-up among the admissible keys beside the MFMAs as K == 2 does (two_smallest on the
// elements AFTER the gate's select, so an inadmissible train is neither winner nor runner-up) and forms, per query of a
// forward problem (p < n_forward, uniform over the workgroup and read in the epilogue only),
//   keep = runner-up present ? 64 * d1 < ratio * d2 : GATED        (integers; a lone train inside a gate is unique)
// then the cap on the winner.  Reversed problems keep their unfiltered 1-NN keys.  keys and rivals are [nprob, q_stride].
//   the train-range split stays: the two smallest merge across splits with vector atomics on the two words of a query,
//     old = atomicMin(&best, b); atomicMin(&rival, max(old, b)); atomicMin(&rival, s);
//     with (b, s) a split's two smallest.  Keys are unique per train, so the minima do not depend on the order of arrival.
//     `best` ends as the smallest b.  Every b that is not that one reaches `rival`: by its own split when it arrives above
//     the current best (max(old, b) = b; best only falls, so it never wins later), or by the split that displaces it
//     (max(old, b) = old).  The overall winner arrives below everything and is never displaced, so it is never pushed.
//     The overall runner-up is either another split's b or the winning split's s, and both kinds are pushed: the end state
//     is the exact two smallest, the bits of the unsplit loop.  The rule and the cap are then one elementwise pass over
//     (best, rival) (ratio_finish_kernel); with nsplit == 1 they are fused into the epilogue here and the pass is skipped.
// Built with -mllvm -amdgpu-mfma-vgpr-form (csrc/Makefile): the accumulators live in VGPRs, no v_accvgpr_read per element.
// KEEP THE MFMA SEQUENCE BRANCH-FREE.  A first version with a wave-uniform `if` around every MFMA returned a wrong key in
// ~8 % of launches under load.  Cause (found from the ISA in round 4): a result of the 8-pass
// v_mfma_i32_32x32x32_i8 may not be touched by a VALU / LDS / VMEM instruction for 12 wait states, there is no hardware
// interlock, and ROCm 7.2's hazard recogniser measures that distance wrongly across the if-diamonds conditional MFMAs
// create (a block first reached through the longer path is not revisited through the shorter one): such forms compile to
// paths with 6 - 10 wait states instead of 12, taken exactly when a wave's second query tile is dead.  Too few wait
// states is a timing-dependent stale read -- hence "only under load".  scripts/check_mfma_hazards.py measures every path
// of this file's ISA itself and tests/test_mfma_isa.py fails the CPU suite when an edit brings such a path (or
// v_accvgpr moves, or a branch inside an accumulation chain) back.
constexpr int kMmaTrainTile = 128;                  // trains per LDS tile
constexpr int kMmaRowPitch = 272;                   // bytes per unpacked train row (256 + 16)
constexpr int32_t kMmaInvalid7 = 1 << 24;           // base7 of a row without a train
constexpr int32_t kMmaInvalid = 1 << 30;            // "no train seen yet" in the wide partial key
typedef int v4i32 __attribute__((ext_vector_type(4)));
typedef int v16i32 __attribute__((ext_vector_type(16)));

// the two smallest of {b, s, k} given b <= s
__device__ __forceinline__ void two_smallest(int32_t& b, int32_t& s, int32_t k) {
  s = max(min(b, s), min(max(b, s), k));  // median of three (v_med3_i32)
  b = min(b, k);
}

// keep(i) of the ratio rule and the cap, on final keys: the one text of the fused epilogue and of ratio_finish_kernel
template <bool GATED>
__device__ __forceinline__ uint32_t ratio_filter(uint32_t k1, uint32_t k2, uint32_t ratio, uint32_t max_distance) {
  if (k1 == SOSVO_KEY_NONE) return k1;
  const uint32_t d1 = k1 >> SOSVO_KEY_SHIFT, d2 = k2 >> SOSVO_KEY_SHIFT;
  const bool keep = k2 == SOSVO_KEY_NONE ? GATED : 64u * d1 < ratio * d2;
  return keep && d1 <= max_distance ? k1 : SOSVO_KEY_NONE;
}

// (q_pos ... max_distance are read by the GATED form only; n_forward by the GATED and the RATIO forms; ratio and rivals by
// the RATIO form, whose K is 1: one key per query in each of keys and rivals)
// CYC (match_hamming_gated_cyclic_mfma_kernel<QT>, sosvo_match_hamming_gated_cyclic): the u side of the
// gate is cyclic with period W -- d = fabs(u_t - u_q) passes iff d <= max_du or d >= wrap_du, wrap_du = W - max_du made once
// on the host: one more double comparison and an OR beside the existing one, still nothing that depends on the accumulators.
template <int QT, int K, bool GATED, bool DV, bool RATIO = false, bool CYC = false>
__device__ __forceinline__ void match_hamming_mfma_body(
    const uint4* __restrict__ q_desc, const uint4* __restrict__ t_desc, const float2* __restrict__ q_pos,
    const float2* __restrict__ t_pos, const int32_t* __restrict__ nq, const int32_t* __restrict__ nt,
    const int32_t* __restrict__ q_slot, const int32_t* __restrict__ t_slot, int n_forward, int q_stride, int t_stride, int nsplit,
    double min_dv, double max_du, uint32_t max_distance, uint32_t ratio, uint32_t* __restrict__ keys,
    uint32_t* __restrict__ rivals, double wrap_du = 0.0) {
  static_assert(!GATED || K == 1, "the gated search stores one key per query");
  static_assert(!CYC || (GATED && !RATIO), "the cyclic gate is a form of the gated search");
  static_assert(!RATIO || K == 1, "the ratio form stores one key per query in keys and one in rivals");
  constexpr bool TWO = K == 2 || RATIO;  // track the runner-up
  SOSVO_LATENCY_BOUND_PRIO();
  __shared__ __attribute__((aligned(16))) uint8_t tile[kMmaTrainTile * kMmaRowPitch];
  __shared__ __attribute__((aligned(16))) int32_t base7[kMmaTrainTile];
  __shared__ __attribute__((aligned(16))) double tu[GATED ? kMmaTrainTile : 2];
  __shared__ __attribute__((aligned(16))) double tv[GATED && DV ? kMmaTrainTile : 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 31, half = lane >> 5;
  const int p = blockIdx.x;
  const int qs = q_slot ? q_slot[p] : p, ts = t_slot ? t_slot[p] : p;
  const int nqp = min(nq[qs], q_stride), ntp = min(nt[ts], t_stride);
  const double vsign = GATED && p >= n_forward ? -1.0 : 1.0;  // uniform over the workgroup
  constexpr int kQPerWg = (kThreads / 64) * 32 * QT;
  const int q0 = blockIdx.y * kQPerWg;
  if (q0 >= nqp) return;  // uniform over the workgroup
  const int tiles = (ntp + kMmaTrainTile - 1) / kMmaTrainTile;
  const int tiles_per = (tiles + nsplit - 1) / nsplit;
  const int tb = blockIdx.z * tiles_per * kMmaTrainTile;
  const int te = min(ntp, tb + tiles_per * kMmaTrainTile);
  if (nsplit > 1 && tb >= te) return;  // keys were pre-set to NONE

  // ---- this wave's queries: unpacked B operands (-16 per set bit) and, when gated, positions, resident
  v4i32 bq[QT][8];
  int32_t pq[QT];
  int32_t best[QT], second[QT];
  double qu[QT], qv[QT];
  // (a wave whose first tile lies beyond the query count sits out the contraction; a dead SECOND tile is computed on a
  // repeated row and never stored: no branch inside the MFMA sequence)
  const bool wave_live = q0 + wave * QT * 32 < nqp;  // wave-uniform
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const int qi = q0 + (wave * QT + t) * 32 + col;
    const size_t row = (size_t)qs * q_stride + (qi < nqp ? qi : q0);
    const uint4 a = q_desc[row * 2 + 0], b = q_desc[row * 2 + 1];
    if constexpr (GATED) {
      const float2 pos = q_pos[row];
      qu[t] = (double)pos.x;
      qv[t] = vsign * (double)pos.y;
    }
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    int32_t pc = 0;
#pragma unroll
    for (int kb = 0; kb < 8; ++kb) {
      pc += __popc(w[kb]);
      const uint32_t y = half ? w[kb] : w[kb] << 4;
      uint32_t n[4];
#pragma unroll
      for (int sft = 0; sft < 4; ++sft) {
        const uint32_t m = (y >> sft) & 0x10101010u;
        n[sft] = (m << 4) - m;  // 0x10 -> 0xF0 = -16 per byte (no carry between bytes)
      }
      bq[t][kb] = v4i32{(int)n[0], (int)n[1], (int)n[2], (int)n[3]};
    }
    pq[t] = pc;
    best[t] = kMmaInvalid;
    second[t] = kMmaInvalid;
  }

  const uint4* tsrc = t_desc + (size_t)ts * t_stride * 2;
  const float2* tpsrc = GATED ? t_pos + (size_t)ts * t_stride : nullptr;
  for (int t0 = tb; t0 < te; t0 += kMmaTrainTile) {
    const int lim = min(kMmaTrainTile, te - t0);
    const int nrb = (lim + 31) >> 5;  // 32-row blocks that hold a train
    __syncthreads();
    // unpack the train tile (16 per set bit): item = (train j, dword kb) -> 32 bytes (both lane halves)
    for (int it = tid; it < nrb * 32 * 8; it += kThreads) {
      const int j = it >> 3, kb = it & 7;
      const uint32_t x = j < lim ? reinterpret_cast<const uint32_t*>(tsrc + (size_t)(t0 + j) * 2)[kb] : 0u;
      uint4 lo, hi;
      lo.x = (x << 4) & 0x10101010u;
      lo.y = (x << 3) & 0x10101010u;
      lo.z = (x << 2) & 0x10101010u;
      lo.w = (x << 1) & 0x10101010u;
      hi.x = x & 0x10101010u;
      hi.y = (x >> 1) & 0x10101010u;
      hi.z = (x >> 2) & 0x10101010u;
      hi.w = (x >> 3) & 0x10101010u;
      uint4* dst = reinterpret_cast<uint4*>(tile + j * kMmaRowPitch + kb * 32);
      dst[0] = lo;
      dst[1] = hi;
    }
    for (int j = tid; j < nrb * 32; j += kThreads) {
      int32_t v = kMmaInvalid7;
      float2 pos = make_float2(0.0f, 0.0f);  // (a row without a train: its base7 loses whatever the gate says)
      if (j < lim) {
        const uint4 a = tsrc[(size_t)(t0 + j) * 2 + 0], b = tsrc[(size_t)(t0 + j) * 2 + 1];
        const int32_t pc = __popc(a.x) + __popc(a.y) + __popc(a.z) + __popc(a.w) + __popc(b.x) + __popc(b.y) + __popc(b.z) +
                           __popc(b.w);
        v = (pc << 7) + j;
        if constexpr (GATED) pos = tpsrc[t0 + j];
      }
      base7[j] = v;
      if constexpr (GATED) tu[j] = (double)pos.x;
      if constexpr (GATED && DV) tv[j] = vsign * (double)pos.y;
    }
    __syncthreads();
    if (!wave_live) continue;  // (uniform per wave; the barriers above are reached by every wave)
    int32_t b7[QT], s7[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) b7[t] = s7[t] = kMmaInvalid;
    for (int rb = 0; rb < nrb; ++rb) {
      v16i32 acc[QT];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const v4i32 b4 = *reinterpret_cast<const v4i32*>(base7 + rb * 32 + 8 * g + 4 * half);
#pragma unroll
        for (int t = 0; t < QT; ++t) {
          acc[t][4 * g + 0] = b4.x;
          acc[t][4 * g + 1] = b4.y;
          acc[t][4 * g + 2] = b4.z;
          acc[t][4 * g + 3] = b4.w;
        }
      }
      const uint8_t* arow = tile + (rb * 32 + col) * kMmaRowPitch + half * 16;
#pragma unroll
      for (int kb = 0; kb < 8; ++kb) {
        const v4i32 a = *reinterpret_cast<const v4i32*>(arow + kb * 32);
#pragma unroll
        for (int t = 0; t < QT; ++t) acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bq[t][kb], acc[t], 0, 0, 0);
      }
      // the min chain over this lane's 16 (train row, query) elements per query tile, a group of four rows at a time; when
      // gated, an element that fails the gate is replaced by kMmaInvalid first.  A CHAIN min(min(best, a), b) per pair of
      // elements: one v_min3_i32 each (no inline asm here: the compiler's hazard recogniser has to see the reads of the MFMA
      // results to place the wait states)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        double ur[4], vr[4] = {0.0, 0.0, 0.0, 0.0};
        if constexpr (GATED) {
          const int r0 = rb * 32 + 8 * g + 4 * half;
          const double2 u01 = *reinterpret_cast<const double2*>(tu + r0), u23 = *reinterpret_cast<const double2*>(tu + r0 + 2);
          ur[0] = u01.x, ur[1] = u01.y, ur[2] = u23.x, ur[3] = u23.y;
          if (DV) {
            const double2 v01 = *reinterpret_cast<const double2*>(tv + r0), v23 = *reinterpret_cast<const double2*>(tv + r0 + 2);
            vr[0] = v01.x, vr[1] = v01.y, vr[2] = v23.x, vr[3] = v23.y;
          }
        }
#pragma unroll
        for (int t = 0; t < QT; ++t) {
          int32_t e[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            e[r] = acc[t][4 * g + r];
            if constexpr (GATED) {
              bool pass;
              if constexpr (CYC) {
                const double d = fabs(ur[r] - qu[t]);
                pass = d <= max_du || d >= wrap_du;
              } else {
                pass = fabs(ur[r] - qu[t]) <= max_du;
              }
              if (DV) pass = pass && (vr[r] - qv[t] >= min_dv);
              e[r] = pass ? e[r] : kMmaInvalid;
            }
          }
          if (!TWO) {
            b7[t] = min(min(b7[t], e[0]), e[1]);
            b7[t] = min(min(b7[t], e[2]), e[3]);
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) two_smallest(b7[t], s7[t], e[r]);
          }
        }
      }
    }
    // widen the tile's winner(s): ((|t| - 2 q.t) << 7) + row  ->  ((|t| - 2 q.t) << 20) + train index
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      const int32_t kb1 = b7[t] < (1 << 23) ? ((b7[t] >> 7) << SOSVO_KEY_SHIFT) + (t0 + (b7[t] & 127)) : kMmaInvalid;
      if (TWO) {
        const int32_t ks1 = s7[t] < (1 << 23) ? ((s7[t] >> 7) << SOSVO_KEY_SHIFT) + (t0 + (s7[t] & 127)) : kMmaInvalid;
        second[t] = min(max(best[t], kb1), min(second[t], ks1));
      }
      best[t] = min(best[t], kb1);
    }
  }

  // ---- the two lane halves of a column hold the same query: merge, add |q|, apply the cap (gated), store
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const int32_t ob = __shfl_xor(best[t], 32), os = __shfl_xor(second[t], 32);
    const int32_t mb = min(best[t], ob);
    const int32_t ms = min(min(second[t], os), max(best[t], ob));
    const int qi = q0 + (wave * QT + t) * 32 + col;
    if (half == 0 && qi < nqp) {
      uint32_t* out = keys + ((size_t)p * q_stride + qi) * K;
      const uint32_t add = (uint32_t)pq[t] << SOSVO_KEY_SHIFT;
      uint32_t kb1 = mb >= kMmaInvalid ? SOSVO_KEY_NONE : (uint32_t)mb + add;
      if (GATED && kb1 != SOSVO_KEY_NONE && (kb1 >> SOSVO_KEY_SHIFT) > max_distance) kb1 = SOSVO_KEY_NONE;
      if constexpr (RATIO) {
        // (the cap above is the reversed rows' and a no-op at 256; a forward row is capped after the rule)
        const uint32_t raw = mb >= kMmaInvalid ? SOSVO_KEY_NONE : (uint32_t)mb + add;
        const uint32_t ks1 = ms >= kMmaInvalid ? SOSVO_KEY_NONE : (uint32_t)ms + add;
        uint32_t* riv = rivals + (size_t)p * q_stride + qi;
        if (p >= n_forward) {  // uniform over the workgroup: the unfiltered 1-NN key of today
          if (nsplit > 1) atomicMin(out, kb1);
          else out[0] = kb1, riv[0] = ks1;
        } else if (nsplit > 1) {
          const uint32_t old = atomicMin(out, raw);
          atomicMin(riv, max(old, raw));
          atomicMin(riv, ks1);
        } else {
          out[0] = ratio_filter<GATED>(raw, ks1, ratio, max_distance);
          riv[0] = ks1;
        }
      } else if (K == 1 && nsplit > 1) {
        atomicMin(out, kb1);
      } else {
        out[0] = kb1;
        if (K == 2) out[1] = ms >= kMmaInvalid ? SOSVO_KEY_NONE : (uint32_t)ms + add;
      }
    }
  }
}

template <int QT, int K>
__global__ __launch_bounds__(kThreads) void match_hamming_mfma_kernel(
    const uint4* __restrict__ q_desc, const uint4* __restrict__ t_desc, const int32_t* __restrict__ nq,
    const int32_t* __restrict__ nt, const int32_t* __restrict__ q_slot, const int32_t* __restrict__ t_slot,
    int q_stride, int t_stride, int nsplit, uint32_t* __restrict__ keys) {
  match_hamming_mfma_body<QT, K, false, false>(q_desc, t_desc, nullptr, nullptr, nq, nt, q_slot, t_slot, 0, q_stride, t_stride,
                                               nsplit, 0.0, 0.0, 0u, 0u, keys, nullptr);
}

template <int QT, bool DV>
__global__ __launch_bounds__(kThreads) void match_hamming_gated_mfma_kernel(
    const uint4* __restrict__ q_desc, const uint4* __restrict__ t_desc, const float2* __restrict__ q_pos,
    const float2* __restrict__ t_pos, const int32_t* __restrict__ nq, const int32_t* __restrict__ nt,
    const int32_t* __restrict__ q_slot, const int32_t* __restrict__ t_slot, int n_forward, int q_stride, int t_stride, int nsplit,
    double min_dv, double max_du, uint32_t max_distance, uint32_t* __restrict__ keys) {
  match_hamming_mfma_body<QT, 1, true, DV>(q_desc, t_desc, q_pos, t_pos, nq, nt, q_slot, t_slot, n_forward, q_stride, t_stride,
                                           nsplit, min_dv, max_du, max_distance, 0u, keys, nullptr);
}

// (the frame-to-frame form only: no v side)
template <int QT>
__global__ __launch_bounds__(kThreads) void match_hamming_gated_cyclic_mfma_kernel(
    const uint4* __restrict__ q_desc, const uint4* __restrict__ t_desc, const float2* __restrict__ q_pos,
    const float2* __restrict__ t_pos, const int32_t* __restrict__ nq, const int32_t* __restrict__ nt,
    const int32_t* __restrict__ q_slot, const int32_t* __restrict__ t_slot, int n_forward, int q_stride, int t_stride, int nsplit,
    double max_du, double wrap_du, uint32_t max_distance, uint32_t* __restrict__ keys) {
  match_hamming_mfma_body<QT, 1, true, false, false, true>(q_desc, t_desc, q_pos, t_pos, nq, nt, q_slot, t_slot, n_forward, q_stride,
                                                           t_stride, nsplit, -1.0, max_du, max_distance, 0u, keys, nullptr, wrap_du);
}

template <int QT, bool GATED, bool DV>
__global__ __launch_bounds__(kThreads) void match_hamming_ratio_mfma_kernel(
    const uint4* __restrict__ q_desc, const uint4* __restrict__ t_desc, const float2* __restrict__ q_pos,
    const float2* __restrict__ t_pos, const int32_t* __restrict__ nq, const int32_t* __restrict__ nt,
    const int32_t* __restrict__ q_slot, const int32_t* __restrict__ t_slot, int n_forward, int q_stride, int t_stride, int nsplit,
    double min_dv, double max_du, uint32_t max_distance, uint32_t ratio, uint32_t* __restrict__ keys,
    uint32_t* __restrict__ rivals) {
  match_hamming_mfma_body<QT, 1, GATED, DV, true>(q_desc, t_desc, q_pos, t_pos, nq, nt, q_slot, t_slot, n_forward, q_stride,
                                                  t_stride, nsplit, min_dv, max_du, max_distance, ratio, keys, rivals);
}

// The rule and the cap over the merged (best, rival) of a split ratio launch: forward rows only (n rows of q_stride keys).
// A row past its problem's query count still holds the NONE it was pre-set to and stays NONE.
template <bool GATED>
__global__ __launch_bounds__(kThreads) void ratio_finish_kernel(uint32_t* __restrict__ keys, const uint32_t* __restrict__ rivals,
                                                                size_t n, uint32_t ratio, uint32_t max_distance) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) keys[i] = ratio_filter<GATED>(keys[i], rivals[i], ratio, max_distance);
}

// ---- float descriptors (SIFT / SURF / KAZE ...): brute-force L2, cv2.BFMatcher() with its default norm
// (omnistereo/camera_models.py:396).  Not on the VO drivers' path (they use binary descriptors): one wave per 64
// queries, the query rows transposed in LDS (lane-contiguous: conflict-free), the train rows in an LDS tile read as
// broadcasts; the squared differences accumulate in float32 four at a time in index order, as OpenCV's scalar
// normL2Sqr_ does (no contraction), distance = sqrt.  Key = (distance bits << 32 | train index): non-negative floats
// order like their bit patterns, so an unsigned min is "smallest distance, first train index".
constexpr int kL2MaxDim = 128, kL2Tile = 32;
template <int K>
__global__ __launch_bounds__(64) void match_l2_kernel(const float* __restrict__ q, const float* __restrict__ t,
                                                      const int32_t* __restrict__ nq, const int32_t* __restrict__ nt,
                                                      int q_stride, int t_stride, int dim,
                                                      unsigned long long* __restrict__ keys) {
  __shared__ float qs[kL2MaxDim * 64];
  __shared__ __attribute__((aligned(16))) float tile[kL2Tile * kL2MaxDim];
  const int lane = threadIdx.x, p = blockIdx.x;
  const int nqp = min(nq[p], q_stride), ntp = min(nt[p], t_stride);
  const int q0 = blockIdx.y * 64;
  if (q0 >= nqp) {  // uniform: padding rows only -- "absent" is all ones, as include/sosvo.h says
    if (q0 + lane < q_stride)
      for (int j = 0; j < K; ++j) keys[((size_t)p * q_stride + q0 + lane) * K + j] = ~0ULL;
    return;
  }
  const int dimp = (dim + 3) & ~3;  // row pitch in the tile
  const float* qsrc = q + ((size_t)p * q_stride + q0) * dim;
  const int rows = min(64, nqp - q0);
  for (int i = lane; i < rows * dim; i += 64) {  // coalesced read, transposed store
    const int r = i / dim, d = i - r * dim;
    qs[d * 64 + r] = qsrc[i];
  }
  unsigned long long best = ~0ULL, second = ~0ULL;
  const float* tsrc = t + (size_t)p * t_stride * dim;
  for (int t0 = 0; t0 < ntp; t0 += kL2Tile) {
    const int lim = min(kL2Tile, ntp - t0);
    __syncthreads();
    for (int i = lane; i < lim * dim; i += 64) {
      const int r = i / dim, d = i - r * dim;
      tile[r * dimp + d] = tsrc[(size_t)t0 * dim + i];
    }
    __syncthreads();
    if (lane >= rows) continue;  // (the barriers above are reached by every lane)
    for (int j = 0; j < lim; ++j) {
      const float* tr = tile + j * dimp;
      float s = 0.0f;
      int i = 0;
      for (; i <= dim - 4; i += 4) {
        const float4 tv = *reinterpret_cast<const float4*>(tr + i);
        const float v0 = qs[i * 64 + lane] - tv.x, v1 = qs[(i + 1) * 64 + lane] - tv.y;
        const float v2 = qs[(i + 2) * 64 + lane] - tv.z, v3 = qs[(i + 3) * 64 + lane] - tv.w;
        s += (((v0 * v0) + (v1 * v1)) + (v2 * v2)) + (v3 * v3);
      }
      for (; i < dim; ++i) {
        const float v = qs[i * 64 + lane] - tr[i];
        s += v * v;
      }
      const unsigned long long key = ((unsigned long long)__float_as_uint(sqrtf(s)) << 32) | (uint32_t)(t0 + j);
      if (K == 2) second = min(second, max(best, key));
      best = min(best, key);
    }
  }
  if (lane < rows || q0 + lane < q_stride) {  // (rows past the query count keep best = second = all ones)
    unsigned long long* out = keys + ((size_t)p * q_stride + q0 + lane) * K;
    out[0] = best;
    if (K == 2) out[1] = second;
  }
}

// Sort by (distance field, query index): ties on distance keep query order (stable), as Python's sorted() does at
// camera_models.py:444.  One workgroup per problem, two forms with the same result:
// * n <= kSortRankMaxN: rank sort.  The sort key of query i is (distance << 20 | i); its rank is the number of smaller sort
//   keys.  Keys are unique, so ranks are a permutation.  O(n^2 / 64) wave-instructions, but next to no fixed cost.
// * larger n: a stable counting sort over the 12-bit field, O(n).  The histogram is indexed by the field itself; `used` =
//   the largest field below 0xFFF plus one (0: every key is SOSVO_KEY_NONE), and only the bins 0 .. used are scanned, where
//   bin `used` stands for NONE in the placement: its exclusive prefix is the number of keys that are not NONE.  The
//   placement walks the queries 64 at a time in index order (one wave: LDS operations of a wave execute in order, so the
//   running per-bin positions are exact without a barrier).  Inside a chunk a lane's peers are the lanes with the same bin
//   (one ballot per bit of the bin index); a lane's position is the bin's running position plus the peers below it, and
//   the lowest peer advances the running position by the number of peers.
constexpr int kSortRankMaxN = 64;
constexpr int kSortBins = 1 << (32 - SOSVO_KEY_SHIFT);  // 4096 values of the field

// Inclusive prefix sum over the 64 lanes through the DPP operand path: four shifts inside the rows of 16 lanes, then the
// last lane of row 0 / 2 into row 1 / 3 (row_bcast:15) and lane 31 into the upper half (row_bcast:31).
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);  // row_shr:1
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);  // row_shr:2
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);  // row_shr:4
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);  // row_shr:8
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);  // row_bcast:15 into rows 1 and 3
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);  // row_bcast:31 into rows 2 and 3
  return v;
}
__device__ __forceinline__ uint32_t wave_inclusive_max(uint32_t v) {  // (0 is the identity: the shifts fill with zeros)
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false));
  return v;
}

__global__ __launch_bounds__(kThreads) void sort_matches_kernel(const uint32_t* __restrict__ keys,
                                                                const int32_t* __restrict__ nq,
                                                                const int32_t* __restrict__ q_slot, int q_stride,
                                                                int32_t* __restrict__ order) {
  SOSVO_LATENCY_BOUND_PRIO();
  extern __shared__ uint32_t sk[];  // rank form: n4 sort keys; counting form: ceil64(n) fields, 16 bits each
  __shared__ uint32_t bins[kSortBins];
  __shared__ uint32_t wave_used[kThreads / 64], wave_tot[kThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int p = blockIdx.x;
  const int n = min(nq[q_slot ? q_slot[p] : p], q_stride);
  if (n <= 0) return;
  const uint32_t* src = keys + (size_t)p * q_stride;
  int32_t* dst = order + (size_t)p * q_stride;
  if (n <= kSortRankMaxN) {  // uniform
    const int n4 = (n + 3) & ~3;
    if (tid < n4) sk[tid] = tid < n ? ((src[tid] & ~SOSVO_KEY_IDX_MASK) | (uint32_t)tid) : 0xFFFFFFFFu;
    __syncthreads();
    if (tid - lane >= n) return;  // (a whole wave)
    const uint32_t mine = tid < n ? sk[tid] : 0u;
    int rank = 0;
    const uint4* sk4 = reinterpret_cast<const uint4*>(sk);
    for (int j = 0; j < n4 / 4; ++j) {
      const uint4 v = sk4[j];
      rank += (v.x < mine) + (v.y < mine) + (v.z < mine) + (v.w < mine);
    }
    if (tid < n) *reinterpret_cast<int32_t*>(reinterpret_cast<char*>(dst) + ((uint32_t)rank << 2)) = tid;
    return;
  }
  uint16_t* sf = reinterpret_cast<uint16_t*>(sk);
#pragma unroll
  for (int k = 0; k < kSortBins / 4 / kThreads; ++k) reinterpret_cast<uint4*>(bins)[k * kThreads + tid] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();  // (a bin is cleared by one wave and counted in by any)
  {  // fields to LDS (the chunk of the last query filled up with NONE), histogram, largest field below 0xFFF
    const int n64 = (n + 63) & ~63;
    uint32_t used = 0u;
    for (int i = tid; i < n64; i += kThreads) {
      // (a 32-bit lane offset on the problem's scalar base, here and at the stores)
      const uint32_t key = i < n ? *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(src) + ((uint32_t)i << 2)) : SOSVO_KEY_NONE;
      const uint32_t f = key >> SOSVO_KEY_SHIFT;
      sf[i] = (uint16_t)f;
      atomicAdd(&bins[f], 1u);
      used = max(used, (key + (1u << SOSVO_KEY_SHIFT)) >> SOSVO_KEY_SHIFT);  // field + 1, and 0 for the field 0xFFF (wraps)
    }
    used = wave_inclusive_max(used);
    if (lane == 63) wave_used[wid] = used;
  }
  __syncthreads();
  // bins 0 .. used - 1 hold the keys that are not NONE
  const int used = __builtin_amdgcn_readfirstlane((int)max(max(wave_used[0], wave_used[1]), max(wave_used[2], wave_used[3])));
  const int per = (used + kThreads) / kThreads;   // bins per thread for the scan of used + 1 bins: 1 .. 16
  const bool scans = wid * 64 * per <= used;      // uniform per wave: the wave owns a bin of 0 .. used
  uint32_t excl = 0u;
  if (scans) {
    uint32_t sum = 0u;
    for (int k = 0; k < per; ++k) sum += bins[tid * per + k];  // (<= 4095; bins past `used` feed no prefix that is read)
    const uint32_t incl = wave_inclusive_sum(sum);
    excl = incl - sum;
    if (lane == 63) wave_tot[wid] = incl;
  }
  __syncthreads();
  if (scans) {
    for (int w = 0; w < wid; ++w) excl += wave_tot[w];
    for (int k = 0; k < per; ++k) {
      const uint32_t c = bins[tid * per + k];
      bins[tid * per + k] = excl;
      excl += c;
    }
  }
  __syncthreads();
  if (wid != 0) return;
  const int nbits = __builtin_amdgcn_readfirstlane(32 - __clz(used));  // bits of the largest bin index in use (`used` itself: NONE)
  const int nchunk = (n + 63) >> 6;
  uint32_t f = sf[lane];
  for (int c = 0; c < nchunk; ++c) {
    const int b = (int)min(f, (uint32_t)used);
    if (c + 1 < nchunk) f = sf[64 * (c + 1) + lane];  // (in flight while this chunk's masks are taken)
    uint32_t peers_lo = 0xFFFFFFFFu, peers_hi = 0xFFFFFFFFu;
    for (int k = 0; k < nbits; ++k) {
      const int bit = __builtin_amdgcn_sbfe(b, k, 1);  // all ones where the bin has bit k
      const unsigned long long bal = __ballot(bit != 0);
      peers_lo &= ~((uint32_t)bal ^ (uint32_t)bit);
      peers_hi &= ~((uint32_t)(bal >> 32) ^ (uint32_t)bit);
    }
    const uint32_t below = __builtin_amdgcn_mbcnt_hi(peers_hi, __builtin_amdgcn_mbcnt_lo(peers_lo, 0u));
    const uint32_t base = bins[b];
    if (below == 0u) atomicAdd(&bins[b], (uint32_t)(__popc(peers_lo) + __popc(peers_hi)));
    const int i = 64 * c + lane;
    if (i < n) *reinterpret_cast<int32_t*>(reinterpret_cast<char*>(dst) + ((base + below) << 2)) = i;
  }
}

// ---- mutual-consistency filter (cv2.BFMatcher(NORM_HAMMING, crossCheck=True), the commented-out matcher of
// omnistereo/camera_models.py:401).  keys_fwd are the 1-NN keys of the queries, keys_rev those of the same search with the
// roles swapped (both "smallest distance, first index"): query i keeps its key iff the train it chose chose it back.  One
// workgroup per problem, so the count of kept matches needs neither atomics nor a cleared output.  keys_out may be
// keys_fwd: a lane reads the entry it writes, and nothing else of that array.
__global__ __launch_bounds__(kThreads) void cross_check_kernel(const uint32_t* keys_fwd, const uint32_t* __restrict__ keys_rev,
                                                               const int32_t* __restrict__ nq, const int32_t* __restrict__ nt,
                                                               const int32_t* __restrict__ q_slot,
                                                               const int32_t* __restrict__ t_slot, int q_stride, int t_stride,
                                                               uint32_t* keys_out, int32_t* __restrict__ n_kept) {
  __shared__ int wave_kept[kThreads / 64];
  const int tid = threadIdx.x, p = blockIdx.x;
  const int n = min(nq[q_slot ? q_slot[p] : p], q_stride), m = min(nt[t_slot ? t_slot[p] : p], t_stride);
  const uint32_t* fwd = keys_fwd + (size_t)p * q_stride;
  const uint32_t* rev = keys_rev + (size_t)p * t_stride;
  uint32_t* out = keys_out + (size_t)p * q_stride;
  int kept = 0;
  for (int i = tid; i < n; i += kThreads) {
    uint32_t k = fwd[i];
    const uint32_t j = k & SOSVO_KEY_IDX_MASK;
    bool keep = false;
    if (k != SOSVO_KEY_NONE && j < (uint32_t)m) {  // (j < m always holds for keys of sosvo_match_hamming: a bounds guard)
      const uint32_t r = rev[j];
      keep = r != SOSVO_KEY_NONE && (r & SOSVO_KEY_IDX_MASK) == (uint32_t)i;
    }
    out[i] = keep ? k : SOSVO_KEY_NONE;
    kept += keep ? 1 : 0;
  }
  if (!n_kept) return;
  for (int s = 32; s > 0; s >>= 1) kept += __shfl_down(kept, s);
  if ((tid & 63) == 0) wave_kept[tid >> 6] = kept;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int w = 0; w < kThreads / 64; ++w) total += wave_kept[w];
    n_kept[p] = total;
  }
}

// ---- radius match ------------------------------------------------------------------------------------------
// cv2.BFMatcher.radiusMatch (omnistereo/camera_models.py:413, FeatureMatcher.use_radius_match): for every query
// ALL train descriptors within max_distance.  One wave per query: the query sits in 8 VGPRs of every lane, lane l
// tests train rows l, l + 64, ...; hits are appended to the query's LDS list in train order through a ballot
// prefix, and the list (at most `cap` keys) leaves sorted by a rank sort on the packed key (distance, then train
// index).  When more than cap rows match, the cap smallest keys are kept by replacing the list's current maximum.
constexpr int kRadiusCapMax = 512;

__global__ __launch_bounds__(kThreads) void match_radius_kernel(
    const uint4* __restrict__ q_desc, const uint4* __restrict__ t_desc, const int32_t* __restrict__ nq,
    const int32_t* __restrict__ nt, const int32_t* __restrict__ q_slot, const int32_t* __restrict__ t_slot,
    int q_stride, int t_stride, uint32_t max_distance, int cap, uint32_t* __restrict__ keys,
    int32_t* __restrict__ counts) {
  __shared__ uint32_t lists[kThreads / 64][kRadiusCapMax];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int p = blockIdx.x;
  const int qs = q_slot ? q_slot[p] : p, ts = t_slot ? t_slot[p] : p;
  const int nqp = min(nq[qs], q_stride), ntp = min(nt[ts], t_stride);
  const int i = blockIdx.y * (kThreads / 64) + wid;  // wave-uniform
  if (i >= nqp) return;
  uint32_t* list = lists[wid];
  const uint4 qa = q_desc[((size_t)qs * q_stride + i) * 2], qb = q_desc[((size_t)qs * q_stride + i) * 2 + 1];
  const uint4* tb = t_desc + (size_t)ts * t_stride * 2;
  int total = 0, kept = 0;  // wave-uniform
  for (int j0 = 0; j0 < ntp; j0 += 64) {
    const int j = j0 + lane;
    bool hit = false;
    uint32_t key = SOSVO_KEY_NONE;
    if (j < ntp) {
      const uint32_t d = hamming256(qa, qb, tb[2 * (size_t)j], tb[2 * (size_t)j + 1]);
      hit = d <= max_distance;
      key = (d << SOSVO_KEY_SHIFT) | (uint32_t)j;
    }
    unsigned long long bal = __ballot(hit);
    if (!bal) continue;
    const int nh = __popcll(bal);
    total += nh;
    if (kept + nh <= cap) {
      if (hit) list[kept + __popcll(bal & ((1ULL << lane) - 1ULL))] = key;
      kept += nh;
    } else {  // overflow: one hit at a time, each replaces the list's maximum if smaller (rare)
      while (bal) {
        const int src = __ffsll((long long)bal) - 1;
        bal &= bal - 1ULL;
        const uint32_t k1 = (uint32_t)__shfl((int)key, src);
        if (kept < cap) {
          if (lane == 0) list[kept] = k1;
          kept++;
        } else {
          uint32_t mx = 0u;
          int mi = 0;
          for (int e = lane; e < cap; e += 64) {
            const uint32_t v = list[e];
            if (v > mx) {
              mx = v;
              mi = e;
            }
          }
          for (int s = 32; s > 0; s >>= 1) {
            const uint32_t ov = (uint32_t)__shfl_down((int)mx, s);
            const int oi = __shfl_down(mi, s);
            if (ov > mx) {
              mx = ov;
              mi = oi;
            }
          }
          mx = (uint32_t)__shfl((int)mx, 0);
          mi = __shfl(mi, 0);
          if (lane == 0 && k1 < mx) list[mi] = k1;
        }
      }
    }
  }
  // rank sort of the kept keys (unique: the train index is part of the key), KEY_NONE padding
  uint32_t* out = keys + ((size_t)p * q_stride + i) * cap;
  for (int e = lane; e < cap; e += 64) {
    if (e >= kept) out[e] = SOSVO_KEY_NONE;
  }
  for (int e = lane; e < kept; e += 64) {
    const uint32_t v = list[e];
    int rank = 0;
    for (int o = 0; o < kept; ++o) rank += list[o] < v ? 1 : 0;
    out[rank] = v;
  }
  if (lane == 0) counts[(size_t)p * q_stride + i] = total;
}

// The launch plan of the matrix-core kernels: 4 waves x qt tiles of 32 queries per workgroup, and for the 1-NN search the
// train range split over grid.z until ~2k workgroups exist (the split results merge with atomicMin on the packed key, so
// the keys are pre-set to NONE here).
struct MmaPlan {
  int qt, nsplit;
  dim3 grid;
};
int32_t mma_plan(sosvo_ctx* ctx, int nprob, int q_stride, int t_stride, int k, uint32_t* keys, MmaPlan* plan,
                 uint32_t* rivals = nullptr) {  // (rivals: the ratio form's second merge word, k = 1)
  plan->qt = (q_stride >= 1024) ? 2 : 1;
  const int gx = cdiv(q_stride, (kThreads / 64) * 32 * plan->qt);
  plan->nsplit = k == 1 && !ctx->hint_match_unsplit ? std::max(1, std::min(cdiv(2048, gx * nprob), std::min(cdiv(t_stride, kMmaTrainTile), 64))) : 1;
  if (plan->nsplit > 1)
    SOSVO_HIP(ctx, hipMemsetAsync(keys, 0xFF, (size_t)nprob * q_stride * sizeof(uint32_t), ctx->stream));
  if (plan->nsplit > 1 && rivals)
    SOSVO_HIP(ctx, hipMemsetAsync(rivals, 0xFF, (size_t)nprob * q_stride * sizeof(uint32_t), ctx->stream));
  plan->grid = dim3(nprob, gx, plan->nsplit);
  return SOSVO_OK;
}

}  // namespace

extern "C" {

int32_t sosvo_match_hamming(sosvo_ctx* ctx, const uint8_t* q_desc, const uint8_t* t_desc,
                            const int32_t* nq, const int32_t* nt, const int32_t* q_slot,
                            const int32_t* t_slot, int32_t nprob, int32_t q_stride, int32_t t_stride, int32_t k,
                            uint32_t* keys) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, q_desc && t_desc && nq && nt && keys, "null pointer");
  SOSVO_REQUIRE(ctx, k == 1 || k == 2, "k must be 1 or 2");
  SOSVO_REQUIRE(ctx, nprob >= 0 && nprob <= 65535, "nprob out of range");
  SOSVO_REQUIRE(ctx, q_stride > 0 && q_stride <= (1 << SOSVO_KEY_SHIFT), "q_stride out of range");
  SOSVO_REQUIRE(ctx, t_stride > 0 && t_stride <= (1 << SOSVO_KEY_SHIFT), "t_stride out of range");
  SOSVO_REQUIRE(ctx, ((uintptr_t)q_desc & 15) == 0 && ((uintptr_t)t_desc & 15) == 0,
                "descriptor arrays must be 16-byte aligned");
  if (nprob == 0) return SOSVO_OK;
  const uint4* q4 = reinterpret_cast<const uint4*>(q_desc);
  const uint4* t4 = reinterpret_cast<const uint4*>(t_desc);
  MmaPlan plan;
  if (const int32_t rc = mma_plan(ctx, nprob, q_stride, t_stride, k, keys, &plan)) return rc;
  // (the profile labels a launch with its instantiation, as SOSVO_LAUNCH does)
  auto launch = [&](auto kernel, const char* name) {
    SOSVO_LAUNCH_AS(ctx, name, kernel, plan.grid, dim3(kThreads), 0, ctx->stream, q4, t4, nq, nt, q_slot, t_slot, q_stride, t_stride,
                    plan.nsplit, keys);
  };
  if (k == 1) {
    if (plan.qt == 2) launch(match_hamming_mfma_kernel<2, 1>, "(match_hamming_mfma_kernel<2, 1>)");
    else launch(match_hamming_mfma_kernel<1, 1>, "(match_hamming_mfma_kernel<1, 1>)");
  } else {
    if (plan.qt == 2) launch(match_hamming_mfma_kernel<2, 2>, "(match_hamming_mfma_kernel<2, 2>)");
    else launch(match_hamming_mfma_kernel<1, 2>, "(match_hamming_mfma_kernel<1, 2>)");
  }
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

// The argument checks and casts that sosvo_match_hamming_gated, ..._gated_cyclic and ..._ratio have in common, over the
// parameter names they share.  Each entry point runs them in the order in which its checks have always fired: the first
// failing one decides the message.
#define MATCH_SIZES_OK(ctx)                                                                                    \
  SOSVO_REQUIRE(ctx, nprob >= 0 && nprob <= 65535, "nprob out of range");                                      \
  SOSVO_REQUIRE(ctx, n_forward >= 0 && n_forward <= nprob, "n_forward out of range (0..nprob)");               \
  SOSVO_REQUIRE(ctx, q_stride > 0 && q_stride <= (1 << SOSVO_KEY_SHIFT), "q_stride out of range");             \
  SOSVO_REQUIRE(ctx, t_stride > 0 && t_stride <= (1 << SOSVO_KEY_SHIFT), "t_stride out of range")
#define MATCH_MAX_DISTANCE_OK(ctx) SOSVO_REQUIRE(ctx, max_distance >= 0 && max_distance <= 256, "max_distance out of range (0..256)")
#define MATCH_GATED_HEAD_OK(ctx)                                                                         \
  SOSVO_REQUIRE(ctx, q_desc && t_desc && q_pos && t_pos && nq && nt && keys, "null pointer");            \
  MATCH_SIZES_OK(ctx);                                                                                   \
  MATCH_MAX_DISTANCE_OK(ctx)
#define MATCH_DESC_ALIGNED(ctx) \
  SOSVO_REQUIRE(ctx, ((uintptr_t)q_desc & 15) == 0 && ((uintptr_t)t_desc & 15) == 0, "descriptor arrays must be 16-byte aligned")
#define MATCH_POS_ALIGNED(ctx) SOSVO_REQUIRE(ctx, ((uintptr_t)q_pos & 7) == 0 && ((uintptr_t)t_pos & 7) == 0, "position arrays must be 8-byte aligned")
#define MATCH_CASTS                                                                                             \
  const uint4 *q4 = reinterpret_cast<const uint4*>(q_desc), *t4 = reinterpret_cast<const uint4*>(t_desc);      \
  const float2 *qp = reinterpret_cast<const float2*>(q_pos), *tp = reinterpret_cast<const float2*>(t_pos)

int32_t sosvo_match_hamming_gated(sosvo_ctx* ctx, const uint8_t* q_desc, const uint8_t* t_desc, const float* q_pos,
                                  const float* t_pos, const int32_t* nq, const int32_t* nt, const int32_t* q_slot,
                                  const int32_t* t_slot, int32_t nprob, int32_t n_forward, int32_t q_stride, int32_t t_stride,
                                  double min_dv, double max_du, int32_t max_distance, uint32_t* keys) {
  SOSVO_ENTER(ctx);
  MATCH_GATED_HEAD_OK(ctx);
  SOSVO_REQUIRE(ctx, min_dv == min_dv && max_du == max_du, "min_dv / max_du must not be NaN");
  MATCH_DESC_ALIGNED(ctx);
  MATCH_POS_ALIGNED(ctx);
  if (nprob == 0) return SOSVO_OK;
  MATCH_CASTS;
  MmaPlan plan;
  if (const int32_t rc = mma_plan(ctx, nprob, q_stride, t_stride, 1, keys, &plan)) return rc;
  // sv_pixel_gate's switches: the du side is on for max_du > 0, the dv side for min_dv >= 0
  const double du = max_du > 0 ? max_du : HUGE_VAL;
  const bool dv = min_dv >= 0;
  const uint32_t cap = (uint32_t)max_distance;
  auto launch = [&](auto kernel, const char* name) {
    SOSVO_LAUNCH_AS(ctx, name, kernel, plan.grid, dim3(kThreads), 0, ctx->stream, q4, t4, qp, tp, nq, nt, q_slot, t_slot, n_forward,
                    q_stride, t_stride, plan.nsplit, min_dv, du, cap, keys);
  };
  if (plan.qt == 2) {
    if (dv) launch(match_hamming_gated_mfma_kernel<2, true>, "(match_hamming_gated_mfma_kernel<2, true>)");
    else launch(match_hamming_gated_mfma_kernel<2, false>, "(match_hamming_gated_mfma_kernel<2, false>)");
  } else {
    if (dv) launch(match_hamming_gated_mfma_kernel<1, true>, "(match_hamming_gated_mfma_kernel<1, true>)");
    else launch(match_hamming_gated_mfma_kernel<1, false>, "(match_hamming_gated_mfma_kernel<1, false>)");
  }
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

int32_t sosvo_match_hamming_gated_cyclic(sosvo_ctx* ctx, const uint8_t* q_desc, const uint8_t* t_desc, const float* q_pos,
                                         const float* t_pos, const int32_t* nq, const int32_t* nt, const int32_t* q_slot,
                                         const int32_t* t_slot, int32_t nprob, int32_t n_forward, int32_t q_stride,
                                         int32_t t_stride, double max_du, double period, int32_t max_distance, uint32_t* keys) {
  SOSVO_ENTER(ctx);
  MATCH_GATED_HEAD_OK(ctx);
  SOSVO_REQUIRE(ctx, max_du == max_du, "max_du must not be NaN");
  SOSVO_REQUIRE(ctx, period >= 1.0 && period <= 16384.0 && period == floor(period), "the period must be a positive integer up to 16384");
  MATCH_DESC_ALIGNED(ctx);
  MATCH_POS_ALIGNED(ctx);
  if (nprob == 0) return SOSVO_OK;
  MATCH_CASTS;
  MmaPlan plan;
  if (const int32_t rc = mma_plan(ctx, nprob, q_stride, t_stride, 1, keys, &plan)) return rc;
  // the switch is sv_pixel_gate's: the gate is on for max_du > 0; off, both sides pass everything
  const double du = max_du > 0 ? max_du : HUGE_VAL;
  const double wrap = max_du > 0 ? period - max_du : HUGE_VAL;
  const uint32_t cap = (uint32_t)max_distance;
  auto launch = [&](auto kernel, const char* name) {
    SOSVO_LAUNCH_AS(ctx, name, kernel, plan.grid, dim3(kThreads), 0, ctx->stream, q4, t4, qp, tp, nq, nt, q_slot, t_slot, n_forward,
                    q_stride, t_stride, plan.nsplit, du, wrap, cap, keys);
  };
  if (plan.qt == 2) launch(match_hamming_gated_cyclic_mfma_kernel<2>, "(match_hamming_gated_cyclic_mfma_kernel<2>)");
  else launch(match_hamming_gated_cyclic_mfma_kernel<1>, "(match_hamming_gated_cyclic_mfma_kernel<1>)");
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

int32_t sosvo_match_hamming_ratio(sosvo_ctx* ctx, const uint8_t* q_desc, const uint8_t* t_desc, const float* q_pos,
                                  const float* t_pos, const int32_t* nq, const int32_t* nt, const int32_t* q_slot,
                                  const int32_t* t_slot, int32_t nprob, int32_t n_forward, int32_t q_stride, int32_t t_stride,
                                  double min_dv, double max_du, int32_t max_distance, int32_t ratio_64ths, uint32_t* keys,
                                  uint32_t* rivals) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, q_desc && t_desc && nq && nt, "null pointer");
  SOSVO_REQUIRE(ctx, keys && rivals, "keys and rivals are both required");
  SOSVO_REQUIRE(ctx, (q_pos != nullptr) == (t_pos != nullptr), "q_pos and t_pos go together (both NULL: the plain form)");
  const bool gated = q_pos != nullptr;
  SOSVO_REQUIRE(ctx, ratio_64ths >= 1 && ratio_64ths <= 63, "ratio_64ths out of range (1..63)");
  MATCH_SIZES_OK(ctx);
  if (gated) {
    MATCH_MAX_DISTANCE_OK(ctx);
    SOSVO_REQUIRE(ctx, min_dv == min_dv && max_du == max_du, "min_dv / max_du must not be NaN");
    MATCH_POS_ALIGNED(ctx);
  } else {
    SOSVO_REQUIRE(ctx, max_distance == 256, "max_distance must be 256 in the plain form (no positions)");
  }
  MATCH_DESC_ALIGNED(ctx);
  SOSVO_REQUIRE(ctx, ((uintptr_t)keys & 3) == 0 && ((uintptr_t)rivals & 3) == 0, "keys and rivals must be 4-byte aligned");
  if (nprob == 0) return SOSVO_OK;
  MATCH_CASTS;
  MmaPlan plan;
  if (const int32_t rc = mma_plan(ctx, nprob, q_stride, t_stride, 1, keys, &plan, rivals)) return rc;
  const double du = max_du > 0 ? max_du : HUGE_VAL;  // (sv_pixel_gate's switches, as in sosvo_match_hamming_gated)
  const bool dv = gated && min_dv >= 0;
  const uint32_t cap = (uint32_t)max_distance, ratio = (uint32_t)ratio_64ths;
  auto launch = [&](auto kernel, const char* name) {
    SOSVO_LAUNCH_AS(ctx, name, kernel, plan.grid, dim3(kThreads), 0, ctx->stream, q4, t4, qp, tp, nq, nt, q_slot, t_slot, n_forward,
                    q_stride, t_stride, plan.nsplit, min_dv, du, cap, ratio, keys, rivals);
  };
  if (plan.qt == 2) {
    if (!gated) launch(match_hamming_ratio_mfma_kernel<2, false, false>, "(match_hamming_ratio_mfma_kernel<2, false, false>)");
    else if (dv) launch(match_hamming_ratio_mfma_kernel<2, true, true>, "(match_hamming_ratio_mfma_kernel<2, true, true>)");
    else launch(match_hamming_ratio_mfma_kernel<2, true, false>, "(match_hamming_ratio_mfma_kernel<2, true, false>)");
  } else {
    if (!gated) launch(match_hamming_ratio_mfma_kernel<1, false, false>, "(match_hamming_ratio_mfma_kernel<1, false, false>)");
    else if (dv) launch(match_hamming_ratio_mfma_kernel<1, true, true>, "(match_hamming_ratio_mfma_kernel<1, true, true>)");
    else launch(match_hamming_ratio_mfma_kernel<1, true, false>, "(match_hamming_ratio_mfma_kernel<1, true, false>)");
  }
  SOSVO_LAUNCH_CHECK(ctx);
  if (plan.nsplit > 1 && n_forward > 0) {
    const size_t n = (size_t)n_forward * q_stride;
    const dim3 grid((unsigned)((n + kThreads - 1) / kThreads));
    if (gated)
      SOSVO_LAUNCH(ctx, ratio_finish_kernel<true>, grid, dim3(kThreads), 0, ctx->stream, keys, rivals, n, ratio, cap);
    else
      SOSVO_LAUNCH(ctx, ratio_finish_kernel<false>, grid, dim3(kThreads), 0, ctx->stream, keys, rivals, n, ratio, cap);
    SOSVO_LAUNCH_CHECK(ctx);
  }
  return SOSVO_OK;
}

int32_t sosvo_cross_check_matches(sosvo_ctx* ctx, const uint32_t* keys_fwd, const uint32_t* keys_rev, const int32_t* nq,
                                  const int32_t* nt, const int32_t* q_slot, const int32_t* t_slot, int32_t nprob,
                                  int32_t q_stride, int32_t t_stride, uint32_t* keys_out, int32_t* n_kept) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, keys_fwd && keys_rev && nq && nt && keys_out, "null pointer");
  SOSVO_REQUIRE(ctx, nprob >= 0 && nprob <= 65535, "nprob out of range");
  SOSVO_REQUIRE(ctx, q_stride > 0 && q_stride <= (1 << SOSVO_KEY_SHIFT) && t_stride > 0 && t_stride <= (1 << SOSVO_KEY_SHIFT),
                "strides out of range");
  if (nprob == 0) return SOSVO_OK;
  SOSVO_LAUNCH(ctx, cross_check_kernel, dim3(nprob), dim3(kThreads), 0, ctx->stream, keys_fwd, keys_rev, nq, nt, q_slot, t_slot,
               q_stride, t_stride, keys_out, n_kept);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

int32_t sosvo_sort_matches(sosvo_ctx* ctx, const uint32_t* keys, const int32_t* nq, const int32_t* q_slot,
                           int32_t nprob, int32_t q_stride, int32_t* order) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, keys && nq && order, "null pointer");
  SOSVO_REQUIRE(ctx, nprob >= 0 && nprob <= 65535, "nprob out of range");
  SOSVO_REQUIRE(ctx, q_stride > 0 && q_stride <= 16384, "q_stride out of range (max 16384)");
  if (nprob == 0) return SOSVO_OK;
  // the rank form's sort keys (n <= kSortRankMaxN) or the counting form's 16-bit fields, whichever needs more
  const size_t lds_rank = (size_t)((std::min(q_stride, kSortRankMaxN) + 3) & ~3) * sizeof(uint32_t);
  const size_t lds = std::max(lds_rank, (size_t)((q_stride + 63) & ~63) * sizeof(uint16_t));
  dim3 grid(nprob), block(kThreads);
  SOSVO_LAUNCH(ctx,sort_matches_kernel, grid, block, lds, ctx->stream, keys, nq, q_slot, q_stride, order);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

int32_t sosvo_match_radius(sosvo_ctx* ctx, const uint8_t* q_desc, const uint8_t* t_desc, const int32_t* nq,
                           const int32_t* nt, const int32_t* q_slot, const int32_t* t_slot, int32_t nprob,
                           int32_t q_stride, int32_t t_stride, int32_t max_distance, int32_t cap, uint32_t* keys,
                           int32_t* counts) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, q_desc && t_desc && nq && nt && keys && counts, "null pointer");
  SOSVO_REQUIRE(ctx, nprob >= 0 && nprob <= 65535, "nprob out of range");
  SOSVO_REQUIRE(ctx, q_stride > 0 && q_stride <= (1 << SOSVO_KEY_SHIFT) && t_stride > 0 && t_stride <= (1 << SOSVO_KEY_SHIFT),
                "strides out of range");
  SOSVO_REQUIRE(ctx, cap > 0 && cap <= kRadiusCapMax, "cap out of range (1..512)");
  SOSVO_REQUIRE(ctx, max_distance >= 0, "max_distance must be >= 0");
  SOSVO_REQUIRE(ctx, (((uintptr_t)q_desc | (uintptr_t)t_desc) & 15) == 0, "descriptors must be 16-byte aligned");
  if (nprob == 0) return SOSVO_OK;
  SOSVO_LAUNCH(ctx, match_radius_kernel, dim3(nprob, cdiv(q_stride, kThreads / 64)), dim3(kThreads), 0, ctx->stream,
               reinterpret_cast<const uint4*>(q_desc), reinterpret_cast<const uint4*>(t_desc), nq, nt, q_slot, t_slot,
               q_stride, t_stride, (uint32_t)max_distance, cap, keys, counts);
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

int32_t sosvo_match_l2(sosvo_ctx* ctx, const float* q_desc, const float* t_desc, const int32_t* nq, const int32_t* nt,
                       int32_t nprob, int32_t q_stride, int32_t t_stride, int32_t dim, int32_t k, uint64_t* keys) {
  SOSVO_ENTER(ctx);
  SOSVO_REQUIRE(ctx, q_desc && t_desc && nq && nt && keys, "null pointer");
  SOSVO_REQUIRE(ctx, nprob >= 0 && nprob <= 65535, "nprob out of range");
  SOSVO_REQUIRE(ctx, q_stride > 0 && q_stride <= (1 << 20) && t_stride > 0 && t_stride <= (1 << 20), "strides out of range");
  SOSVO_REQUIRE(ctx, dim >= 1 && dim <= kL2MaxDim, "dim out of range (1..128)");
  SOSVO_REQUIRE(ctx, k == 1 || k == 2, "k must be 1 or 2");
  if (nprob == 0) return SOSVO_OK;
  if (k == 1)
    SOSVO_LAUNCH(ctx, match_l2_kernel<1>, dim3(nprob, cdiv(q_stride, 64)), dim3(64), 0, ctx->stream, q_desc, t_desc, nq, nt,
                 q_stride, t_stride, dim, reinterpret_cast<unsigned long long*>(keys));
  else
    SOSVO_LAUNCH(ctx, match_l2_kernel<2>, dim3(nprob, cdiv(q_stride, 64)), dim3(64), 0, ctx->stream, q_desc, t_desc, nq, nt,
                 q_stride, t_stride, dim, reinterpret_cast<unsigned long long*>(keys));
  SOSVO_LAUNCH_CHECK(ctx);
  return SOSVO_OK;
}

}  // extern "C"
