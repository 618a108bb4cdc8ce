/* sosvo_dense_filter.h -- the WLS disparity filter of the dense omnistereo path, an extension of the C
 * ABI in include/sosvo.h with a header of its own: it includes sosvo.h for sosvo_ctx, the status codes and
 * SOSVO_DENSE_CYCLIC_COLUMNS, and sosvo.h does not include it.  The functions live in libsosvo.so beside the others.
 *
 * The reference's tuner controls "Use WLS filter", "WLS lambda" and "WLS sigma" (common_cv.StereoMatchTuner,
 * common_cv.py:498-500 and 675-685) run cv2.ximgproc's DisparityWLSFilter over the map: an edge-aware smoothing and hole
 * filling guided by the left view.  The definition here is the project's own, modelled on that filter (a fast global smoother
 * applied to confidence-weighted disparities); no parity with cv2.ximgproc is claimed.  tests/refwls.py is the same text in
 * numpy, which the device reproduces bit for bit.  Both stages work per frame; no frame sees another.                     */
#ifndef SOSVO_DENSE_FILTER_H
#define SOSVO_DENSE_FILTER_H

#include "sosvo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SOSVO_WLS_MAX_RADIUS 7
#define SOSVO_WLS_MAX_ROLL_PPM 1000000
#define SOSVO_WLS_MAX_ITERS 8
#define SOSVO_WLS_MAX_LAMBDA 1.0e6
#define SOSVO_WLS_WEIGHTS 256

/* A. sosvo_dense_confidence: d16 [n, rows, cols] i16 -> conf_out [n, rows, cols] u8.  All arithmetic is integer.
 *   a. A pixel is valid iff d16 >= 0, as in sosvo_dense_speckle.
 *   b. The window of a pixel is its (2 radius + 1)^2 taps (r + dy, c + dx), |dy|, |dx| <= radius, 0 <= radius <= 7.  Rows
 *      outside the map do not exist.  Columns outside do not exist either, unless SOSVO_DENSE_CYCLIC_COLUMNS is set in flags:
 *      then tap column c + dx is taken modulo cols (a window wider than the map meets a pixel more than once and counts it
 *      each time).
 *   c. Over the valid taps, in int64: m (their count), s1 (the sum of d16), s2 (the sum of d16^2).
 *   d. V = (m s2 - s1^2) / m^2 by floor division: the variance in (1/16 row)^2.
 *   e. conf = max(0, 255 - (255 * roll_ppm * V) / 1000000) (floor division) for a valid pixel, 0 for an invalid one.
 *      0 <= roll_ppm <= 10^6; 1000 is OpenCV's roll-off of 0.001, and 3 its radius.  Nothing overflows int64 in these ranges.
 *   255 inside a smooth surface, falling to 0 at a depth discontinuity (a one-row step: about 239; a ten-row step: 0).
 *
 * SOSVO_ERR_ARG before any launch: d16 or conf_out NULL; rows or cols outside 1 .. 16384; n < 1 or > 32767; radius outside
 * 0 .. 7; roll_ppm outside 0 .. 10^6; unknown flag bits.  Asynchronous on the context's stream; no scratch.            */
int32_t sosvo_dense_confidence(sosvo_ctx* ctx, const int16_t* d16, int32_t n, int32_t rows, int32_t cols, int32_t radius,
                               int32_t roll_ppm, int32_t flags, uint8_t* conf_out);

/* B. sosvo_dense_wls: d16 [n, rows, cols] i16, guide [n, rows, cols] u8 (the gray panorama the map belongs to: the top view),
 * conf [n, rows, cols] u8 or NULL (255 on every valid pixel), mask [rows, cols] u8 or NULL -> d16_out [n, rows, cols] i16 and,
 * if not NULL, planes_out [n, 2, rows, cols] f64: the final numerator and denominator (so that a failing parity test says
 * which stage differs).  weights: a HOST array of 256 doubles, each finite and in [0, 1]; weights[k] is the affinity of two
 * neighbours whose gray values differ by k.  The device evaluates no exponential: the caller makes the table (Python:
 * exp(-k / sigma), once per options value), and it is read before the call returns.
 *
 * Everything below is IEEE double, one rounding per written operation, no fused multiply-add, subnormals honoured.
 *   1. w = (d16 >= 0) ? conf : 0.  Two right-hand sides: N = (double)(w * d16) and D = (double)w, both exact integers.
 *   2. For t = 0 .. iters - 1 (1 <= iters <= 8): lam_t = ((1.5 * lambda) * 4^(iters-1-t)) / (4^iters - 1); solve along every
 *      row of the map, then along every column, replacing N and D each time.
 *   3. One line of n elements with guide values g_i and a right-hand side f:
 *        wl_i = lam_t * weights[|g_i - g_(i-1)|], 0 for i = 0;  wr_i = lam_t * weights[|g_(i+1) - g_i|], 0 for i = n - 1;
 *        b_i = (1 + wl_i) + wr_i,  a_i = -wl_i,  c_i = -wr_i.
 *        Forward:  r_0 = 1 / b_0, c'_0 = c_0 r_0, f'_0 = f_0 r_0;
 *                  r_i = 1 / (b_i - a_i c'_(i-1)), c'_i = c_i r_i, f'_i = (f_i - a_i f'_(i-1)) r_i.
 *        Backward: u_(n-1) = f'_(n-1), u_i = f'_i - c'_i u_(i+1).
 *      One reciprocal per step, shared by all right-hand sides.  The system is (I + lam_t A) u = f with A the weighted graph
 *      Laplacian of the line; its rows sum to 1, so a constant stays constant.
 *   4. With SOSVO_DENSE_CYCLIC_COLUMNS and cols >= 3 the ROW system is the cyclic one (column cols - 1 neighbours column 0),
 *      solved by Sherman-Morrison:
 *        ws = lam_t * weights[|g_0 - g_(n-1)|];  b_0 = (1 + ws) + wr_0;  b_(n-1) = (1 + wl_(n-1)) + ws;
 *        gamma = -b_0;  b_0 <- b_0 - gamma;  b_(n-1) <- b_(n-1) - ((-ws)(-ws)) / gamma;
 *        a third right-hand side (gamma, 0, ..., 0, -ws) in the same sweep gives z beside y;
 *        q = (-ws) / gamma,  vy = y_0 + q y_(n-1),  vz = 1 + (z_0 + q z_(n-1)),  x_i = y_i - z_i (vy / vz).
 *      The columns of the map (the second solve of every iteration) are never cyclic.  With cols < 3 the flag changes nothing.
 *   5. Where D >= 255 * min_weight (min_weight finite and positive): d16_out = clamp(floor(N / D + 0.5), 0, 32767).  Every
 *      other pixel, and every pixel where mask == 0, becomes -1.
 *   6. 0 <= lambda <= 10^6.  With lambda = 0 the filter returns d16 wherever w > 0.
 *   7. d16_out may be d16 itself: the kernels read the map (and conf) once, in step 1.
 * Temporaries (N, D, c' and two f', 40 bytes per pixel, and the table; in the cyclic form a third f', 8 bytes per pixel, and
 * 16 bytes per row) live in the context's scratch.
 *
 * SOSVO_ERR_ARG before any launch: d16, guide, weights or d16_out NULL; rows or cols outside 1 .. 16384; n < 1 or > 32767;
 * lambda not in [0, 10^6] (a NaN included); a table entry that is not finite or not in [0, 1]; iters outside 1 .. 8;
 * min_weight not finite or not positive; unknown flag bits.  Asynchronous on the context's stream.                      */
int32_t sosvo_dense_wls(sosvo_ctx* ctx, const int16_t* d16, const uint8_t* guide, const uint8_t* conf, const uint8_t* mask,
                        int32_t n, int32_t rows, int32_t cols, double lambda, const double* weights, int32_t iters,
                        double min_weight, int32_t flags, int16_t* d16_out, double* planes_out);

#ifdef __cplusplus
}
#endif
#endif /* SOSVO_DENSE_FILTER_H */
