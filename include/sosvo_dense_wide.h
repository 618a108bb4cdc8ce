/* sosvo_dense_wide.h -- dense omnistereo with 16 to 256 disparities, an extension of the C ABI in
 * include/sosvo.h with a header of its own, in the manner of sosvo_dense_filter.h: it includes sosvo.h for sosvo_ctx, the status
 * codes, SOSVO_DENSE_CYCLIC_COLUMNS and SOSVO_DENSE_MAX_P2_EIGHT_PATHS, and sosvo.h does not include it.  The function lives in
 * libsosvo.so beside the others.  The ABI version stays 1.
 *
 * The reference tuner's "num_of_disparities" (common_cv.StereoMatchTuner, common_cv.py:491 and :782): a multiple of 16 from 16
 * to 256, default 64, 240 in the preset for real panoramas; a caller maps it as disparities = tuner.num_of_disparities.  The
 * disparity of a surface at horizontal distance rho is baseline / (rho * pixel_size) rows, so a fixed 64 leaves a blind near
 * range that grows with the panorama's width, and a surface nearer than that does not go missing: it comes out as confident
 * wrong depth.  Fewer than 64 disparities on far scenes move a quarter or half of the volume.
 *
 * Definition.  Steps a to g of sosvo_dense_stereo and the eight paths of sosvo_dense_stereo_paths (include/sosvo.h) hold with
 * D = disparities in place of 64 in exactly four places; tests/refdense_wide.py is the same text in numpy, which the device
 * reproduces bit for bit.
 *   1. The cost volume C (u8) and the aggregated volume S (u16) are [n, rows, cols, D], k-contiguous.
 *      C(r, c, k) = the Hamming distance of the census words of top (r, c) and bottom (r - min_disparity - k, c).
 *   2. In the recurrence L(p, k) = C(p, k) + min(L'(k), L'(k - 1) + P1, L'(k + 1) + P1, min_j L'(j) + P2) - min_j L'(j) over
 *      the predecessor's L', k = 0 has no k - 1 and k = D - 1 has no k + 1; the minimum runs over the D values.
 *   3. The winner k* is the smallest k among the minimal S over the D values.
 *   4. The 1/16-row parabola through S(k* - 1), S(k*), S(k* + 1) is skipped (offset 0) at k* = 0 and at k* = D - 1.
 * Unchanged: the cost is 64 where the bottom row does not exist (a constant of the 62-bit census, not of D); S is u16 with
 * P2 <= 8191 for four paths and P2 <= 8127 for eight, because the bound paths * (64 + P2) does not depend on D; min_disparity
 * is 0 .. 1024, and the largest d16 is (1024 + 255) * 16 + 8 = 20 472; the left-right key is (mS << 14) | r; uniqueness, reach,
 * mask and the left-right check are those of sosvo_dense_stereo.  D > rows is accepted: the disparities that no row can reach
 * cost 64 everywhere.
 *
 * With disparities == 64 the call IS sosvo_dense_stereo_paths: the same launches, the same scratch and the same bytes.
 *
 * S_out: [n, rows, cols, disparities] u16 or NULL (then S lives in the scratch).
 * Temporaries in the context's scratch, bytes per pixel: 8 + 8 (the two views' census words) + D (C) + 2 D (S, without S_out)
 * + 2 (k*, 16 bits: 255 is a winner at D = 256, so 0xFFFF marks a pixel without one) + 4 (the left-right keys, with
 * lr_max >= 0) = 22 + 3 D: 70 at D = 16, 406 at D = 128, 790 at D = 256.  (D = 64 runs the older layout, whose k* is a
 * byte: 8 + 8 + D + 2 D + 1 + 4 = 213.)
 *
 * SOSVO_ERR_ARG before any launch, under this function's name: everything sosvo_dense_stereo_paths refuses (a NULL top, bot or
 * d16_out; rows or cols outside 1 .. 16384; n < 1 or > 32767; P1 < 0, P1 > P2, P2 > 8191; uniqueness outside [0, 100);
 * min_disparity outside [0, 1024]; unknown flag bits; paths other than 4 or 8; paths = 8 with P2 > 8127), then disparities
 * outside 16 .. 256 or not a multiple of 16.  Asynchronous on the context's stream.                                        */
#ifndef SOSVO_DENSE_WIDE_H
#define SOSVO_DENSE_WIDE_H

#include "sosvo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SOSVO_DENSE_WIDE_MIN_DISPARITIES 16
#define SOSVO_DENSE_WIDE_MAX_DISPARITIES 256

int32_t sosvo_dense_stereo_wide(sosvo_ctx* ctx, const uint8_t* top, const uint8_t* bot, int32_t n, int32_t rows, int32_t cols,
                                const uint8_t* mask, int32_t min_disparity, int32_t disparities, int32_t P1, int32_t P2,
                                int32_t uniqueness, int32_t lr_max, int32_t flags, int32_t paths, int16_t* d16_out, uint16_t* S_out);

#ifdef __cplusplus
}
#endif
#endif /* SOSVO_DENSE_WIDE_H */
