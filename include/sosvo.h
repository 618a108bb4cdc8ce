/*
 * sosvo.h -- C ABI of libsosvo.so, the MI355X (gfx950) front end of the single-camera
 * SOS visual-odometry hot path.
 *
 * The reference (ubuntuslave/vo_single_camera_sos) is pure Python and has no FFI of its
 * own: its "native boundary" is the set of Python call sites into cv2 / pyopengv.  Every
 * entry point below names the reference call site (file:line under the reference tree)
 * whose arithmetic it replaces.  The ctypes binding a maintainer would add on the
 * reference side is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every function returns SOSVO_OK (0) or a negative sosvo_status; the message of the
 *     last failure on a context is sosvo_last_error(ctx);
 *   - all data pointers are DEVICE pointers owned by the caller (e.g. torch tensors'
 *     data_ptr()); the library never allocates result memory and keeps no pointer
 *     after a call returns, except the scratch workspace owned by the context;
 *   - every call enqueues work on the context's HIP stream and returns without
 *     synchronising (graph-capturable); counts live in device memory so no stage needs
 *     a host round trip;
 *   - one context per host thread; a context is bound to (device, stream);
 *   - "batched, fixed capacity" layout: problem p of a batch owns rows
 *     [p*stride, p*stride + count[p]) of an array, count[p] <= stride.
 *   - a descriptor is 32 bytes (256 bits); a match key is the u32
 *     (hamming_distance << 20) | train_index, so that unsigned order on keys is the
 *     reference's order: smaller distance first, then the FIRST (lowest) train index.
 */
#ifndef SOSVO_H
#define SOSVO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sosvo_ctx sosvo_ctx;

typedef enum {
  SOSVO_OK = 0,
  SOSVO_ERR_ARG = -1,      /* bad argument (null pointer, size out of range) */
  SOSVO_ERR_HIP = -2,      /* a HIP runtime call failed */
  SOSVO_ERR_NODEVICE = -3, /* no gfx950 device / device index out of range */
  SOSVO_ERR_CAPACITY = -4  /* a fixed capacity would be exceeded */
} sosvo_status;

#define SOSVO_DESC_BYTES 32
#define SOSVO_KEY_SHIFT 20
#define SOSVO_KEY_IDX_MASK 0xFFFFFu
#define SOSVO_KEY_NONE 0xFFFFFFFFu

/* ---- context ------------------------------------------------------------------------ */

/* Version of this ABI (bumped on any signature change). */
int32_t sosvo_abi_version(void);

/* The descriptor test pattern cv2.ORB_create(...).compute uses (omnistereo/camera_models.py:1682, :1765;
 * pose_est_tools.py:520, :553): OpenCV's learned table bit_pattern_31_, 256 tests x (x0, y0, x1, y1) = [512, 2] int8
 * points, |coordinate| <= 13, written to HOST memory (1024 bytes).  It is the `pattern` argument of sosvo_describe_orb*,
 * sosvo_detect_orb* and the batch entry points (which take it in device memory: copy it once).  Any other [512, 2] table
 * with |coordinate| <= 16 is accepted there too (the Python package keeps a seeded one as `orb_pattern.seeded_pattern()`).
 * No context needed. */
int32_t sosvo_orb_bit_pattern_31(int8_t* pattern_host);

/* Create a context on `device`; `stream` is a hipStream_t (0 = the null stream; pass
 * torch.cuda.current_stream().cuda_stream to order with torch work). */
int32_t sosvo_create(sosvo_ctx** out, int32_t device, void* stream);
int32_t sosvo_destroy(sosvo_ctx* ctx);
int32_t sosvo_set_stream(sosvo_ctx* ctx, void* stream);
/* Hints that change scheduling, never results.  SOSVO_HINT_SHARED_DEVICE (value != 0): kernels of OTHER contexts / streams
 * run on the device at the same time (a batch split over streams): the register-filling median kernel then keeps to three
 * workgroups per CU so that the others find wave slots (+1.3 % on the three-stream step, -2.5 % for that kernel alone).
 * sosvo_frame_pair_batch_streams sets it on its internal contexts itself. */
#define SOSVO_HINT_SHARED_DEVICE 1
/* SOSVO_HINT_SCORE_FP64_ONLY (value != 0): the RANSAC scoring kernel skips its single-precision first tier (which decides
 * an inlier test only where a proven rounding bound allows and leaves the rest to double precision) and evaluates every
 * test in double precision, as rounds 1 - 3 did.  Same counts, bit for bit (tests/test_gpu_ransac.py compares the two
 * forms); ~1.6 x the kernel's time.  For A/B measurements (scripts/score_tiers.py). */
#define SOSVO_HINT_SCORE_FP64_ONLY 2
/* SOSVO_HINT_MATCH_UNSPLIT (value != 0): sosvo_match_hamming(k = 1), sosvo_match_hamming_gated and sosvo_match_hamming_ratio
 * walk the whole train range in one workgroup per query tile instead of splitting it over workgroups that merge with atomics
 * (small problem counts: the live driver, sequence mode at window 1).  Same keys and rivals, bit for bit
 * (tests/test_gpu_ratio_test.py compares the two forms).  For A/B measurements (scripts/bench_ratio_test.py); not passed on
 * to the internal contexts of sosvo_frame_pair_batch_streams. */
#define SOSVO_HINT_MATCH_UNSPLIT 3
/* SOSVO_HINT_ROLLING_NARROW (value != 0): the rolling image kernels run in their one-column-per-lane form at every image
 * width: the 7x7 blur of sosvo_gauss7, sosvo_describe_orb* and the ORB detector's levels (otherwise four columns per lane
 * from 8 columns on) and the corner response of sosvo_detect_gft (otherwise two).  Same bytes, same keypoints
 * (tests/test_gpu_blur_wide.py and tests/test_gpu_response_wide.py compare the forms).  For A/B measurements; passed on to the internal contexts of sosvo_frame_pair_batch_streams. */
#define SOSVO_HINT_ROLLING_NARROW 4
int32_t sosvo_set_hint(sosvo_ctx* ctx, int32_t hint, int32_t value);
int32_t sosvo_synchronize(sosvo_ctx* ctx);
const char* sosvo_last_error(const sosvo_ctx* ctx);

/* HIP-event timer on the context's stream (used by bench.py for per-kernel durations):
 * start/stop record events; elapsed synchronises on the stop event and returns ms. */
int32_t sosvo_timer_start(sosvo_ctx* ctx);
int32_t sosvo_timer_stop(sosvo_ctx* ctx);
int32_t sosvo_timer_elapsed_ms(sosvo_ctx* ctx, float* ms);

/* Per-kernel HIP-event profile on the context's stream: while enabled, every kernel launch of
 * every entry point is bracketed by an event pair (up to 16384 launches since the last enable).
 * sosvo_profile_enable(on) also clears the record.  sosvo_profile_get synchronises on entry i and
 * returns the kernel's label and its duration in ms.                                            */
int32_t sosvo_profile_enable(sosvo_ctx* ctx, int32_t on);
int32_t sosvo_profile_count(sosvo_ctx* ctx);
int32_t sosvo_profile_get(sosvo_ctx* ctx, int32_t i, char* name_out, int32_t name_cap, float* ms);

/* Test hook: fills the context's internal scratch memory (response maps, sort keys, RANSAC hypotheses, blurred images;
 * the internal sub-contexts of sosvo_frame_pair_batch_streams included) with `byte`, on the context's stream(s).  No
 * entry point may read scratch it has not written in the same call, so results must not depend on this.            */
int32_t sosvo_debug_fill_scratch(sosvo_ctx* ctx, int32_t byte);

/* ---- K1: unwrap (a1 + a2) ---------------------------------------------------------------------
 * Replaces Panorama.get_panoramic_image's cv2.remap(omni, map_x, map_y, INTER_LINEAR,
 * BORDER_CONSTANT, 0) (omnistereo/panorama.py:293) for both mirrors of every frame, with
 * OmniStereoModel.get_fully_masked_images' bitwise_and (camera_models.py:2991-2996) folded into
 * the bilinear taps (a masked-out source pixel reads 0, exactly as masking the image first).
 *   omni  [nframes, H, W, 3] u8 (BGR)
 *   masks [2, H, W] u8, non-zero = pixel belongs to that mirror's annulus; NULL = no masking
 *   map_x, map_y [2, rows, cols] f32: Panorama.world2cam_LUT_map_x/y cast to float32 (:291-292);
 *       NaN entries give the border colour 0
 *   pano  [2, nframes, rows, cols, 3] u8 -- VIEW-MAJOR: image i = view * nframes + frame
 * Arithmetic: coordinates rounded to 1/32 px (ties to even), weights (32-fx)(32-fy),
 * (sum + 512) >> 10; taps outside the image read 0.  1 <= H, W <= 16384, every such frame size.  */
int32_t sosvo_unwrap(sosvo_ctx* ctx, const uint8_t* omni, const uint8_t* masks, const float* map_x,
                     const float* map_y, int32_t nframes, int32_t H, int32_t W, int32_t rows,
                     int32_t cols, uint8_t* pano);

/* Table-driven form of K1 for the batched path (identical results): sosvo_unwrap_prepare folds the
 * float maps, the 1/32-px rounding, the border test and the annulus masks into a packed table
 * [2, rows, cols, 2] u32 once per model (an opaque 8-byte entry per panorama pixel: the byte offset of the first
 * tap and the four blend weights; the table is specific to (H, W), and frames larger than 4 MB take a slower,
 * still exact entry format); sosvo_unwrap_table then unwraps nframes frames with one 8-byte table load and two
 * unaligned 8-byte tap loads per panorama pixel.
 * FRAME SIZE of the table form: 1 <= H, W <= 16384 and 3 * W * (H - 1) >= 8, i.e. 8 bytes must follow the start of the
 * frame's second row (the kernels load 8 bytes there for a panorama pixel without a valid tap).  That excludes one-row
 * frames and 2 x 2; (2, 3), (3, 2) and (4, 1) are the smallest accepted.  sosvo_unwrap_prepare and every entry point that
 * reads frames through the table refuse other sizes with SOSVO_ERR_ARG: sosvo_unwrap_table,
 * sosvo_unwrap_median_gray[_rows], sosvo_frame_pair_batch[_streams[_enqueue]] and sosvo_sequence_front_end[_slots].  The
 * map form sosvo_unwrap above has no such loads.                                                                  */
int32_t sosvo_unwrap_prepare(sosvo_ctx* ctx, const uint8_t* masks, const float* map_x, const float* map_y,
                             int32_t H, int32_t W, int32_t rows, int32_t cols, uint32_t* table);
int32_t sosvo_unwrap_table(sosvo_ctx* ctx, const uint8_t* omni, const uint32_t* table, int32_t nframes,
                           int32_t H, int32_t W, int32_t rows, int32_t cols, uint8_t* pano);

/* ---- K2 + K3: median blur + gray --------------------------------------------------------------
 * Replaces cv2.medianBlur(pano, ksize) (omnistereo/camera_models.py:1711, pose_est_tools.py:528;
 * ksize 11 for the SOS frames, 0 = none for RGB-D) followed by cv2.cvtColor(BGR2GRAY)
 * (camera_models.py:1714, or the conversion ORB does internally).  Exact k x k median per channel
 * with replicated border, then (1868 B + 9617 G + 4899 R + 8192) >> 14.
 *   img [nimg, rows, cols, 3] u8 -> gray [nimg, rows, cols] u8.  ksize in {0, 1, 3, 5, 11}.       */
int32_t sosvo_median_gray(sosvo_ctx* ctx, const uint8_t* img, int32_t nimg, int32_t rows,
                          int32_t cols, int32_t ksize, uint8_t* gray);
/* K1 + K2 + K3 in one kernel for the batched path (identical results to sosvo_unwrap_table followed by
 * sosvo_median_gray on its output): every lane unwraps its source pixel from the table on the fly, so the
 * colour panoramas (camera_models.py:2991-2996 -> :1711 -> :1714) are never written to HBM.
 *   omni [nframes, H, W, 3] u8, table from sosvo_unwrap_prepare -> gray [2 * nframes, rows, cols] u8
 *   (view-major).  ksize in {3, 5, 11}; 0 / 1 = no median: the pixel is unwrapped and converted to gray at once.
 *   H, W: the frame size of the table form (see sosvo_unwrap_prepare), for this call and the _rows form below.     */
int32_t sosvo_unwrap_median_gray(sosvo_ctx* ctx, const uint8_t* omni, const uint32_t* table, int32_t nframes,
                                 int32_t H, int32_t W, int32_t rows, int32_t cols, int32_t ksize, uint8_t* gray);

/* The same with the output restricted to the rows a consumer can reach: row_range = int32 [2][2] in DEVICE memory
 * (view-major: first row, last row + 1 of the top and of the bottom panoramas), written by sosvo_gray_rows_needed;
 * NULL = all rows (sosvo_unwrap_median_gray).  Rows outside a view's range are neither computed nor written (the
 * caller's buffer keeps what it held); inside, the result is sosvo_unwrap_median_gray's bit for bit.  (ksize 0 / 1 writes
 * every row and does not read row_range.) */
int32_t sosvo_unwrap_median_gray_rows(sosvo_ctx* ctx, const uint8_t* omni, const uint32_t* table, int32_t nframes,
                                      int32_t H, int32_t W, int32_t rows, int32_t cols, int32_t ksize,
                                      const int32_t* row_range, uint8_t* gray);

/* Rows of the gray panoramas that goodFeaturesToTrack on the azimuthal masks (camera_models.py:1739: the response at
 * the masked pixels and its 3x3 dilation, i.e. gray within 3 rows of a masked row) and ORB.compute on its keypoints
 * (camera_models.py:1765: keypoints edge <= y < rows - edge inside the masks, rotated pattern on the 7x7-blurred
 * image) can reach, per mask set: mask_bits [nsets, rows, cols] u32 -> row_range [nsets][2] int32 (device): first row,
 * last row + 1 (0, 0 for an empty set).  Model constant: compute once per (masks, edge, pattern, angle). */
int32_t sosvo_gray_rows_needed(sosvo_ctx* ctx, const uint32_t* mask_bits, int32_t nsets, int32_t rows, int32_t cols,
                               int32_t nmask, int32_t edge, const int8_t* pattern, float cos_a, float sin_a,
                               int32_t* row_range);

/* ---- K4: goodFeaturesToTrack per azimuthal mask (a4, the reference's default detector) ---------
 * Replaces cv2.goodFeaturesToTrack(image, maxCorners, qualityLevel, minDistance, mask, useHarris=False)
 * as called per mask from OmniCamModel.detect_sparse_features_on_panorama
 * (omnistereo/camera_models.py:1739, :1778) and RGBDFrame.detect_sparse_features (pose_est_tools.py:544).
 *   gray      [nimg, rows, cols] u8 (the median-blurred gray panorama, camera_models.py:1711-1714)
 *   mask_bits [nsets, rows, cols] u32: bit m set = the pixel belongs to azimuthal mask m (masks may
 *             overlap); image i uses set i / images_per_maskset (one set per mirror)
 * Problem p = image * nmask + mask.  Per problem: min-eigenvalue map (Sobel 3, block 3, reflect-101,
 * float32), maxVal over the mask, threshold quality * maxVal, 3x3 dilation NMS excluding the 1-px
 * image border, descending sort (ties: higher address first), greedy min-distance on a cell grid,
 * stop at max_corners (<= 0: no limit) or at the output capacity `cap`.  quality > 0; quality >= 1 is accepted as by
 * OpenCV and yields no corners (threshold >= maximum).  Only positive responses can become corners (with 0 < quality
 * the threshold is positive wherever the mask's maximum is; a mask whose maximum is <= 0 has no corners).
 *   kp [nimg*nmask, cap, 2] f32 (x, y) in acceptance order, n [nimg*nmask] i32,
 *   status [nimg*nmask] i32 (optional): bit 0 = more candidates than the selection keeps (4096; 16384 when
 *   cap > 1024: the large-mask variant for whole-image detection, e.g. the RGB-D frames) -- the result is then
 *   goodFeaturesToTrack on the CAND strongest candidates, a prefix of the full result (CAND = 4096 or 16384, a function
 *   of cap alone; the strongest in the order of the sort: descending response, higher address first among equal
 *   responses; when max_corners or cap is reached inside them the result is the full one); bit 1 = mask too large for the on-chip grid (3584 / 15872 cells of
 *   minDistance^2 pixels) and more than 1024 corners wanted, or more than 1024 corners were the THIRD of their grid
 *   cell (possible from minDistance ~30 px on; up to 1024 of them are kept exactly in an overflow list).
 * rows, cols <= 65535 (and rows * cols < 2^28): the candidates travel as y << 16 | x. */
int32_t sosvo_detect_gft(sosvo_ctx* ctx, const uint8_t* gray, const uint32_t* mask_bits, int32_t nimg,
                         int32_t images_per_maskset, int32_t rows, int32_t cols, int32_t nmask,
                         double quality, double min_distance, int32_t max_corners, int32_t cap,
                         float* kp, int32_t* n, int32_t* status);

/* The first half of sosvo_detect_gft on its own, for tests of the corner-response kernel: the masks' bounding boxes and the
 * response kernel, whose outputs are copied out of the context's workspace (stream-ordered device-to-device copies).
 *   geometry (HOST, int32 [6], always written): strip width, strips per row, row chunks, rows per chunk, record slots per
 *     region (wcap), number of regions = nimg * strips * chunks.  Region r = (image * chunks + chunk) * strips + strip holds
 *     the positive 3x3 local maxima of the response inside some mask among the columns strip * width .. + width - 1 and
 *     the rows chunk * rows_per_chunk .. + rows_per_chunk - 1, except the image's outermost rows and columns, row-major
 *     and by ascending x within a row.
 *   With cand_out, wcnt_out and mstat_out all NULL only geometry is written (the sizes to allocate).  Otherwise (DEVICE):
 *   cand_out u32 [regions, wcap, 2]: (response bits, y << 16 | x), the first min(wcnt, wcap) of a region are valid;
 *   wcnt_out u32 [regions]: candidates found in the region (may exceed wcap);
 *   mstat_out u32 [nimg * nmask, 5]: [0] the mask's largest response in the order-preserving integer form (0 = no pixel;
 *     f >= 0 -> bits | 0x80000000, f < 0 -> ~bits), [1..4] the bounding box fields of sosvo_detect_gft's selection.
 * The geometry depends on the sizes, the context's hints and the library version, never on the image content. */
int32_t sosvo_detect_gft_candidates(sosvo_ctx* ctx, const uint8_t* gray, const uint32_t* mask_bits, int32_t nimg,
                                    int32_t images_per_maskset, int32_t rows, int32_t cols, int32_t nmask, int32_t* geometry,
                                    uint32_t* cand_out, uint32_t* wcnt_out, uint32_t* mstat_out);

/* ---- K6a on its own: the 7x7 sigma-2 Gaussian of the descriptor stage ---------------------------
 * out = the blur of gray in 8.8 fixed point (weights 18 34 49 54 49 34 18 / 256 per axis, reflect-101 border, horizontal
 * sums kept exactly, (v + 32768) >> 16 after the vertical pass): image i is read at gray + i * img_stride and written at
 * out + i * out_stride, rows * cols bytes each (strides >= rows * cols; nothing between or beyond the images is read or
 * written).  row_range: int32 [2][2] in DEVICE memory as for sosvo_describe_orb_rows (view-major, nimg even; rows outside a
 * view's range are not written), NULL = all rows.  gray and out must not overlap. */
int32_t sosvo_gauss7(sosvo_ctx* ctx, const uint8_t* gray, int32_t nimg, int32_t rows, int32_t cols, int64_t img_stride,
                     uint8_t* out, int64_t out_stride, const int32_t* row_range);

/* ---- K6: ORB descriptors on provided keypoints (a4) --------------------------------------------
 * Replaces ORB_create(nfeatures).compute(image, keypoints) (omnistereo/camera_models.py:1765, :1785;
 * pose_est_tools.py:553): keypoints nearer than `edge` (31) px to the border are REMOVED (kp and n
 * are compacted in place, order kept), the image is blurred 7x7 sigma 2 (8.8 fixed point), and the
 * 256 pair tests of `pattern` [512,2] i8 (device) are evaluated at offsets rotated by the keypoint
 * angle (cos_a, sin_a as float32: the GFT path gives every keypoint angle -1 degree) and rounded.
 * Problem p = image * nmask + mask as above.  desc [nimg*nmask, cap, 32] u8, 8 tests per byte, LSB first. */
int32_t sosvo_describe_orb(sosvo_ctx* ctx, const uint8_t* gray, int32_t nimg, int32_t rows, int32_t cols,
                           int32_t nmask, int32_t cap, float* kp, int32_t* n, float cos_a, float sin_a,
                           const int8_t* pattern, int32_t edge, uint8_t* desc);

/* The same with the blur restricted to the rows a descriptor can read: row_range = int32 [2][2] in DEVICE memory as written
 * by sosvo_gray_rows_needed for the same masks / edge / pattern (view-major: first row, last row + 1; image i belongs to
 * view i / (nimg / 2)); NULL = all rows (sosvo_describe_orb).  Descriptors are sosvo_describe_orb's bit for bit.
 * Precondition made safe: a keypoint whose patch rows y - R .. y + R (R = the rotated pattern's radius) leave the rows
 * [first + 3, last + 1 - 3) of its view's range (inner ends only; an end at the image border does not count) would read
 * rows that were never blurred -- it is REMOVED like a keypoint within `edge` of the border.  Keypoints inside the masks
 * the range was derived from are never affected. */
int32_t sosvo_describe_orb_rows(sosvo_ctx* ctx, const uint8_t* gray, int32_t nimg, int32_t rows, int32_t cols,
                                int32_t nmask, int32_t cap, float* kp, int32_t* n, float cos_a, float sin_a,
                                const int8_t* pattern, int32_t edge, const int32_t* row_range, uint8_t* desc);

/* ---- sub-pixel refinement of detected keypoints (cv2.cornerSubPix, the companion of goodFeaturesToTrack) ----------
 * Refines kp [nimg*nmask, cap, 2] f32 IN PLACE on gray [nimg, rows, cols] u8, the image the detector saw; n, the order and
 * the rows of kp at and beyond n[p] are untouched.  Problem p = image * nmask + mask as above.  The rule is cornerSubPix
 * restated in exact integers.  Per keypoint: c0 = the position as given (f32 -> double), c = c0; each iteration
 *   1. rounds the sampling centre to 1/32 px: xq = floor(32 c.x + 0.5), yq likewise;
 *   2. takes the (2 half + 3)^2 bilinear samples at centre + (j - half - 1, i - half - 1) px as integers,
 *      S = (32 - fy) ((32 - fx) p00 + fx p01) + fy ((32 - fx) p10 + fx p11) <= 255 * 1024; pixel coordinates are
 *      clamped (replicated) to the columns [0, cols) and to the rows [first, last + 1) of the view's row_range;
 *   3. over the (2 half + 1)^2 window, in int64: gx = S[i+1][j+2] - S[i+1][j], gy = S[i+2][j+1] - S[i][j+1],
 *      m = (w[i] w[j]) >> 8 with the table of sosvo_subpix_weights, px = j - half, py = i - half,
 *      a += gx gx m, b += gx gy m, c2 += gy gy m, b1 += gx gx m px + gx gy m py, b2 += gx gy m px + gy gy m py
 *      (each sum < 2^55: exact, whatever the order of summation);
 *   4. solves in double, every sum converted once: det = a c2 - b b; det == 0 ends the iteration and c stays; otherwise
 *      c' = (xq / 32 + (c2 b1 - b b2) / det, yq / 32 + (a b2 - b b1) / det), err = |c' - c|^2;
 *   5. if !(|c'.x - c0.x| <= half && |c'.y - c0.y| <= half) the result is c0 (a NaN reverts too); otherwise c = c', and the
 *      iteration ends after max_iter iterations or when err <= eps^2.
 * The output is (float)c.  A keypoint with a non-finite coordinate is left as it is.  Reads stay within 2 half + 2 px of c0.
 *   half 2..5, max_iter >= 1, eps >= 0 (cv2's TermCriteria(COUNT + EPS, max_iter, eps)); otherwise SOSVO_ERR_ARG.
 *   row_range: int32 [2][2] in DEVICE memory as for sosvo_describe_orb_rows (view-major, nimg even); NULL = all rows.  A
 *   range is cut to the image and holds at least one row.  With the range the gray image was computed for, keypoints that
 *   sosvo_describe_orb_rows kept never touch the clamp (pattern radius + 3 >= 2 half + 2).
 * sosvo_subpix_weights: the table w[k] = floor(256 exp(-((k - half) / half)^2) + 0.5), k = 0 .. 2 half, written to HOST memory
 * (2 half + 1 int32); what the kernel uses, so that a reference on another libm cannot differ in the last bit.  ctx may be
 * NULL (it only receives the error message); no GPU needed.                                                          */
int32_t sosvo_subpix_weights(sosvo_ctx* ctx, int32_t half, int32_t* w_host);
int32_t sosvo_refine_subpix(sosvo_ctx* ctx, const uint8_t* gray, int32_t nimg, int32_t rows, int32_t cols, int32_t nmask,
                            int32_t cap, float* kp, const int32_t* n, int32_t half, int32_t max_iter, double eps,
                            const int32_t* row_range);

/* ---- pyramidal Lucas-Kanade tracking (cv2.calcOpticalFlowPyrLK, the call the reference carries commented out beside its
 * matcher, omnistereo/camera_models.py:3070) restated in exact integers ---------------------------------------------------
 * sosvo_gray_pyramid builds the levels 1 .. levels - 1 of nimg gray images [nimg, rows, cols] u8; level 0 is the caller's
 * buffer and is not copied.  rows_{l+1} = (rows_l + 1) / 2, cols likewise; a pixel of level l + 1 is
 *   (sum over i, j in -2 .. 2 of k_i k_j L_l[clamp(2 y + i)][clamp(2 x + j)] + 128) >> 8,  k = (1, 4, 6, 4, 1).
 * The border is REPLICATED (clamp), not OpenCV's reflect-101: a row range can clamp the same way.
 *   row_range: int32 [2][2] in DEVICE memory as for sosvo_refine_subpix (view-major, nimg even; image i belongs to view
 *   i / (nimg / 2)): rows [first, last + 1) of level 0, cut to the image and to at least one row; NULL = all rows.  The range
 *   of level l + 1 is [(r0_l + 1) / 2, max((r1_l + 1) / 2, that + 1)), cut to the level's rows as at level 0 (a range on the
 *   last row of an even level); only those rows are computed and written, and the reads of level l clamp into ITS range.
 *   Rows outside keep what the buffer held.
 *   pyr: the levels back to back, level l as [nimg, rows_l, cols_l]; sosvo_gray_pyramid_bytes gives its size (HOST out
 *   pointer; ctx may be NULL, no GPU needed).  levels 1 .. 4 (1: nothing to do, pyr may be NULL); rows, cols <= 16384.
 *
 * sosvo_track_lk: problem p < nprob tracks the points prev_pts[p, 0 .. n[p]) ([nprob, cap, 2] f32, level-0 pixels) from
 * image prev_img[p] to image next_img[p] of ONE pyramid set (gray = level 0, pyr = sosvo_gray_pyramid's output for the same
 * nimg, rows, cols, levels, row_range; prev_img, next_img: [nprob] int32 in DEVICE memory, as the matcher's slots; a problem
 * with an index outside [0, nimg) is ignored).  Outputs next_pts [nprob, cap, 2] f32, status [nprob, cap] u8 (1 = tracked),
 * err [nprob, cap] f32; rows at and beyond n[p] are untouched.  Per point, p = the start (f32 -> double), g = the guess:
 *   g = p, or next_pts on entry with SOSVO_LK_INITIAL_FLOW; a non-finite p or g: status 0, next = prev, err 0.
 *   g_L-1 = g / 2^(L-1); then for l = L-1 .. 0, on level l (cols_l columns, rows [r0_l, r1_l) of the view's range):
 *   1. the template centre p / 2^l is rounded to 1/32 px (tq = floor(32 x + 0.5), base tq >> 5, fraction tq & 31).  A rounded
 *      centre outside [0, cols_l - 1] x [r0_l, r1_l - 1]: the point is LOST at level 0; above it the level is skipped.
 *   2. T = the (2 half + 3)^2 integer bilinear samples around it (weights (32 - f) and f, <= 255 * 1024; coordinates clamped
 *      to the columns and the row range).  Scharr gradients over the (2 half + 1)^2 window:
 *      gx = 3 (T[i-1][j+1] - T[i-1][j-1]) + 10 (T[i][j+1] - T[i][j-1]) + 3 (T[i+1][j+1] - T[i+1][j-1]), gy transposed;
 *      A = sum gx^2, B = sum gx gy, C = sum gy^2 in int64 (each < 441 * 2^44 < 2^53).
 *   3. in double, every sum converted once: det = A C - B B; e = (A + C - sqrt((A - C)(A - C) + 4 B B)) / (N 2^31),
 *      N = (2 half + 1)^2, the square root correctly rounded -- OpenCV's minimum eigenvalue per pixel in gray levels squared.
 *      det == 0 or e < min_eig: LOST at level 0, the level is skipped above it (the guess is carried down).
 *   4. up to max_iter times: the guess is rounded to 1/32 px (gq); a rounded guess outside the level (as in 1., with the NEXT
 *      image's row range) loses the point at level 0 and ends the level's iteration above it; J = the (2 half + 1)^2 samples
 *      of the next image around it; d = J - T, b1 = sum d gx, b2 = sum d gy in int64 (< 2^49);
 *      dx = -32 (C b1 - B b2) / det, dy = -32 (A b2 - B b1) / det; g = gq / 32 + (dx, dy).
 *      Stop when dx^2 + dy^2 <= eps^2; from the second iteration on also when |dx + previous dx| < 0.01 and the same in y
 *      (OpenCV's oscillation stop): then g -= (dx, dy) / 2.
 *   5. l > 0: g_{l-1} = 2 g_l.  l = 0: the guess is rounded once more (outside: LOST), err = sum |J - T| / (1024 N) there,
 *      next = (float)g, status 1.  A LOST point: status 0, err 0, next = (float) of the guess it was lost with.
 *   half 2 .. 10, max_iter 1 .. 30, eps >= 0, min_eig >= 0 (OpenCV's default 1e-4), cap <= 4096, levels 1 .. 4; otherwise
 *   SOSVO_ERR_ARG.  No wrap-around of the panorama's columns without SOSVO_LK_CYCLIC_COLUMNS (below).
 *   back (optional, [nprob, cap, 2] f32) with fb_max > 0: the forward-backward check.  Every point with status 1 is tracked
 *   back from next_pts (no initial guess) in image next_img[p] to image prev_img[p]; back receives that position (next_pts for
 *   the points whose status was 0) and the status is cleared where the way back is lost or |back - prev|^2 > fb_max^2
 *   (differences of the float32 values in double).
 *
 * CYCLIC COLUMNS (a panorama is a full circle: column W = cols is column 0 again).
 * sosvo_gray_pyramid_cyclic is sosvo_gray_pyramid with the column index (2 x + j) mod cols_l in place of the clamp; rows and
 * row ranges exactly as above, clamp included.  It needs cols % 2^(levels - 1) == 0, so that level l has exactly cols >> l
 * columns and is one period; otherwise SOSVO_ERR_ARG.  Same sizes, same buffer (sosvo_gray_pyramid_bytes).
 * sosvo_track_lk with SOSVO_LK_CYCLIC_COLUMNS in flags (it combines with SOSVO_LK_INITIAL_FLOW; pyr = the cyclic pyramid) is
 * the rule above with these changes and no others:
 *   a. wherever a position is rounded to the 1/32-px grid (the template centre, every guess, the final rounding) the x
 *      component tq_x = floor(32 x + 0.5) is reduced to tq_x mod (32 cols_l), in [0, 32 cols_l).  "Outside the level" is a
 *      matter of the rows only; a non-finite value, or |32 x + 0.5| >= 2^40, is outside as it is above.
 *   b. every sample's two column taps are (bx + j) mod cols_l and (bx + j + 1) mod cols_l: base cols_l - 1 with a fraction
 *      blends into column 0.
 *   c. the step is taken from the wrapped rounded guess: g = gq / 32 + (dx, dy); g_{l-1} = 2 g_l as above.
 *   d. the x written is w = g.x - W floor(g.x / W) in double, cast to float32; a float that equals W is written as 0.  The
 *      same for the guess a LOST point is written with.  y, status and err are unchanged.
 *   e. in the forward-backward check the x part of |back - prev|^2 is the cyclic distance min(d, W - d), d = |back.x - prev.x|,
 *      with prev.x as given: the check assumes starts within one period of [0, W) (d <= W); a start further out is tracked
 *      as a position on the circle but its check fails.
 *   Same window sizes, same sums, same bounds.  It needs cols % 2^(levels - 1) == 0 and at least 2 half + 3 columns on the
 *   top level (cols >> (levels - 1): the template fits one period, no column is sampled twice in a row of it); otherwise
 *   SOSVO_ERR_ARG.  Points whose windows stay away from columns 0 and W - 1 on every level get the bits of the plain call.
 *   Flag value 2 is not a flag and stays refused.                                                                       */
#define SOSVO_LK_INITIAL_FLOW 1
#define SOSVO_LK_CYCLIC_COLUMNS 4
int32_t sosvo_gray_pyramid_bytes(sosvo_ctx* ctx, int32_t nimg, int32_t rows, int32_t cols, int32_t levels, int64_t* bytes);
int32_t sosvo_gray_pyramid(sosvo_ctx* ctx, const uint8_t* gray, int32_t nimg, int32_t rows, int32_t cols, int32_t levels,
                           const int32_t* row_range, uint8_t* pyr);
int32_t sosvo_gray_pyramid_cyclic(sosvo_ctx* ctx, const uint8_t* gray, int32_t nimg, int32_t rows, int32_t cols, int32_t levels,
                                  const int32_t* row_range, uint8_t* pyr);
int32_t sosvo_track_lk(sosvo_ctx* ctx, const uint8_t* gray, const uint8_t* pyr, int32_t nimg, int32_t rows, int32_t cols,
                       int32_t levels, const int32_t* row_range, const int32_t* prev_img, const int32_t* next_img, int32_t nprob,
                       int32_t cap, const float* prev_pts, const int32_t* n, int32_t half, int32_t max_iter, double eps,
                       double min_eig, int32_t flags, float* next_pts, uint8_t* status, float* err, float* back, double fb_max);

/* ---- K5: ORB keypoint detection per azimuthal mask (a4, feature_detection_method "ORB") ----------
 * Replaces cv2.ORB_create(nfeatures=N).detect(image, mask) (omnistereo/camera_models.py:1640, :1755;
 * pose_est_tools.py:478, :547) for all azimuthal masks of all images at once: 8 levels x 1.2, per-level
 * quotas, FAST-9/16 (threshold 20) with 3x3 NMS, 31-px border, (resized) mask, best 2 n_l by FAST score,
 * Harris response, best n_l, intensity-centroid orientation; see vo_single_camera_sos_amd/csrc/orb.hip.
 *   sosvo_orb_pyramid_pixels(rows, cols): pixels of one image's 8-level pyramid (host helper)
 *   sosvo_orb_mask_pyramid: mask_bits [nsets, rows, cols] u32 -> mask_pyr [nsets, pyramid_pixels] u32,
 *       every mask resized level by level (kept where > 254); call once per model
 *   sosvo_detect_orb: gray [nimg, rows, cols] u8 -> kp4 [nimg*nmask, cap, 4] f32 = (x, y in level-0
 *       coordinates, angle in degrees, level), resp [nimg*nmask, cap] f32 (Harris), n [nimg*nmask] i32;
 *       keypoints ordered by level, then response descending, then (y, x).  Per (problem, level) any number of FAST
 *       maxima is handled; only a retainBest set (best 2 n_l by FAST score, ties kept) of more than 2048 keypoints --
 *       thousands tied at the threshold score -- is cut to 2048 (which of the tied ones go on is then unspecified).
 * ---- K6': ORB descriptors for oriented multi-level keypoints
 * Replaces .compute(image, keypoints) on ORB's own keypoints (camera_models.py:1765): keypoints within
 * 31 px of the level-0 border are removed (kp4 / n compacted in place), each level is blurred 7x7 sigma 2,
 * the pattern is rotated by the keypoint's angle.  desc [nimg*nmask, cap, 32] u8; kp_xy (optional)
 * [nimg*nmask, cap, 2] f32 receives the compacted (x, y) for the matching stages.
 * sosvo_describe_orb_levels builds its own pyramid (all 8 levels: the keypoints may come from anywhere).
 *   sosvo_detect_describe_orb: detect, then compute, as the reference does (camera_models.py:1755, :1765), in ONE call
 *       that builds ONE pyramid -- only as far as a keypoint can come from (levels with a quota and more than the 31-px
 *       border) -- and shares it between the two halves.  Same outputs as sosvo_detect_orb followed by
 *       sosvo_describe_orb_levels, bit for bit; cap <= 2048.                                                        */
int64_t sosvo_orb_pyramid_pixels(int32_t rows, int32_t cols);
int32_t sosvo_orb_mask_pyramid(sosvo_ctx* ctx, const uint32_t* mask_bits, int32_t nsets, int32_t rows,
                               int32_t cols, int32_t nmask, uint32_t* mask_pyr);
int32_t sosvo_detect_orb(sosvo_ctx* ctx, const uint8_t* gray, const uint32_t* mask_pyr, int32_t nimg,
                         int32_t images_per_maskset, int32_t rows, int32_t cols, int32_t nmask,
                         int32_t nfeatures, int32_t cap, float* kp4, float* resp, int32_t* n);
int32_t sosvo_describe_orb_levels(sosvo_ctx* ctx, const uint8_t* gray, int32_t nimg, int32_t rows,
                                  int32_t cols, int32_t nmask, int32_t cap, float* kp4, int32_t* n,
                                  const int8_t* pattern, uint8_t* desc, float* kp_xy);
int32_t sosvo_detect_describe_orb(sosvo_ctx* ctx, const uint8_t* gray, const uint32_t* mask_pyr, int32_t nimg,
                                  int32_t images_per_maskset, int32_t rows, int32_t cols, int32_t nmask,
                                  int32_t nfeatures, int32_t cap, float* kp4, float* resp, int32_t* n,
                                  const int8_t* pattern, uint8_t* desc, float* kp_xy);

/* ---- FAST as a detector of its own (a4, feature_detection_method "FAST") -------------------------------
 * Replaces cv2.FastFeatureDetector_create() + setNonmaxSuppression(True) + .detect(image, mask)
 * (omnistereo/camera_models.py:1664-1666, :1755; pose_est_tools.py:506-508) for all azimuthal masks of all
 * images: FAST-9/16 with `threshold` (OpenCV default 10) on the whole image, 3x3 non-maximum suppression on the
 * corner score, keypoints where the mask bit is set, in raster order (rows, then x).  The descriptors then come
 * from sosvo_describe_orb with the fixed angle -1 degree, as for GFT keypoints (camera_models.py:1765).
 *   kp [nimg*nmask, cap, 2] f32 (x, y), n [nimg*nmask] i32, status (optional): 1 = more than cap corners (the
 *   first cap in raster order are kept).                                                                      */
int32_t sosvo_detect_fast(sosvo_ctx* ctx, const uint8_t* gray, const uint32_t* mask_bits, int32_t nimg,
                          int32_t images_per_maskset, int32_t rows, int32_t cols, int32_t nmask,
                          int32_t threshold, int32_t cap, float* kp, int32_t* n, int32_t* status);

/* ---- AGAST as a detector (a4, feature_detection_method "AGAST") -------------------------------------------
 * Replaces cv2.AgastFeatureDetector_create() + setNonmaxSuppression(True) + .detect(image, mask)
 * (omnistereo/camera_models.py:1670-1671, :1755; pose_est_tools.py:508-509): OAST 9/16 -- the corner set and response of
 * FAST-9/16 at `threshold` (OpenCV default 10) -- with AGAST's own non-maximum suppression (one maximum per block of
 * vertically / horizontally touching corners), keypoints where the mask bit is set, raster order.  Same arguments and
 * outputs as sosvo_detect_fast; status bit 1: more than 16384 corners in an image (the rest is dropped); rows <= 1024. */
int32_t sosvo_detect_agast(sosvo_ctx* ctx, const uint8_t* gray, const uint32_t* mask_bits, int32_t nimg,
                           int32_t images_per_maskset, int32_t rows, int32_t cols, int32_t nmask,
                           int32_t threshold, int32_t cap, float* kp, int32_t* n, int32_t* status);

/* ---- K7: brute-force Hamming matching ------------------------------------------------
 * Replaces cv2.BFMatcher(NORM_HAMMING).match / .knnMatch as called from
 * omnistereo/camera_models.py:442 and :420 (FeatureMatcher.match, :404-446).
 *
 * Problem p < nprob matches the query rows of block qs = q_slot ? q_slot[p] : p against the
 * train rows of block ts = t_slot ? t_slot[p] : p (the slots let many problems share one
 * descriptor store, e.g. frame-to-frame problems index frames).  For each query row i < nq[qs]:
 *   keys[(p*q_stride + i)*k + 0] = min over j < nt[ts] of (hamming(q_i, t_j) << 20 | j)
 *   keys[(p*q_stride + i)*k + 1] = second smallest such key            (only if k == 2)
 * Missing neighbours (nt[ts] < k) are SOSVO_KEY_NONE.  Rows i >= nq[qs] are unspecified.
 * q_desc: [*, q_stride, 32] u8, t_desc: [*, t_stride, 32] u8 (16-byte aligned); nq, nt: i32
 * counts per block; q_slot, t_slot: [nprob] i32 or NULL.  k is 1 or 2.  strides <= 2^20.   */
int32_t sosvo_match_hamming(sosvo_ctx* ctx, const uint8_t* q_desc, const uint8_t* t_desc,
                            const int32_t* nq, const int32_t* nt, const int32_t* q_slot,
                            const int32_t* t_slot, int32_t nprob, int32_t q_stride,
                            int32_t t_stride, int32_t k, uint32_t* keys);

/* The 1-NN search under the pixel gates (guided matching: the search along the epipolar band, where sosvo_match_hamming
 * searches everywhere and leaves the geometry to the assemble stages).  Blocks, slots, strides and counts as in
 * sosvo_match_hamming; q_pos [*, q_stride, 2] f32 and t_pos [*, t_stride, 2] f32 (8-byte aligned) hold the pixel (u, v)
 * of every descriptor row, indexed like the descriptors, finite values.  With the float32 positions converted to double,
 *   gate(i, j) = (max_du > 0 ? fabs(u_t - u_q) <= max_du : true) && (min_dv >= 0 ? v_t - v_q >= min_dv : true)
 * which is the gate of the assemble stages (sosvo_stereo_assemble with the train the top and the query the bottom view:
 * min_dv = stereo_min_disp, max_du = stereo_max_hdiff; sosvo_f2f_assemble: min_dv < 0, max_du = f2f_max_hdiff), evaluated in
 * double exactly as they do; the azimuth gets no wrap-around, as there.  Problems p >= n_forward are REVERSED: their v side
 * reads v_q - v_t >= min_dv (the same gate seen from the swapped roles; the u side is symmetric), so a step's forward
 * problems and their role-swapped twins for sosvo_cross_check_matches run as one launch; n_forward = nprob: none is.
 * For each query row i < nq[qs]:
 *   keys[p*q_stride + i] = min over j < nt[ts] with gate(i, j) of (hamming(q_i, t_j) << 20 | j)
 *                        = SOSVO_KEY_NONE if no j passes, or if the winner's distance exceeds max_distance
 * max_distance: 0 .. 256 (256: no cap; the winner has the smallest admissible distance, so the cap acts on it alone).
 * Rows i >= nq[qs] are unspecified.  1-NN only.  With both gate sides disabled and max_distance = 256 the keys are those
 * of sosvo_match_hamming(k = 1), bit for bit.  sosvo_sort_matches puts SOSVO_KEY_NONE last and the assemble stages count
 * the keys that are not SOSVO_KEY_NONE, as after sosvo_cross_check_matches. */
int32_t sosvo_match_hamming_gated(sosvo_ctx* ctx, const uint8_t* q_desc, const uint8_t* t_desc, const float* q_pos,
                                  const float* t_pos, const int32_t* nq, const int32_t* nt, const int32_t* q_slot,
                                  const int32_t* t_slot, int32_t nprob, int32_t n_forward, int32_t q_stride, int32_t t_stride,
                                  double min_dv, double max_du, int32_t max_distance, uint32_t* keys);

/* sosvo_match_hamming_gated in its frame-to-frame form (no v side) with the CYCLIC u side: the
 * positions are columns of a panorama of `period` columns, a full circle.  With d = fabs(u_t - u_q) in double,
 *   gate(i, j) = max_du > 0 ? (d <= max_du || d >= period - max_du) : true
 * where period - max_du is formed once, in double, on the host.  Where that difference is exact (max_du a multiple of 2^-38)
 * this is sosvo_f2f_assemble_cyclic's d <= max_du || period - d <= max_du; where it rounds, the two can differ for a pair whose
 * d equals the rounded difference, and the assemble behind the matcher decides (it gates again).
 * period: a positive integer up to 16384, otherwise SOSVO_ERR_ARG.  Everything else (blocks, slots, reversed problems, the
 * cap, the train-range split) as in sosvo_match_hamming_gated; with max_du <= 0 the keys are those of that call with both
 * sides disabled. */
int32_t sosvo_match_hamming_gated_cyclic(sosvo_ctx* ctx, const uint8_t* q_desc, const uint8_t* t_desc, const float* q_pos,
                                         const float* t_pos, const int32_t* nq, const int32_t* nt, const int32_t* q_slot,
                                         const int32_t* t_slot, int32_t nprob, int32_t n_forward, int32_t q_stride,
                                         int32_t t_stride, double max_du, double period, int32_t max_distance, uint32_t* keys);

/* Lowe's distinctiveness ("ratio") rule fused into the 1-NN search (omnistereo/camera_models.py:421-423: knnMatch(k = 2) and
 * m[0].distance < m[1].distance * 0.75).  Arguments as in sosvo_match_hamming_gated, and two forms:
 *   q_pos == t_pos == NULL  the PLAIN form: every train j < nt[ts] is admissible; min_dv / max_du are ignored and
 *                           max_distance must be 256
 *   both given              the GATED form: the admissible trains are those that pass gate(i, j) of
 *                           sosvo_match_hamming_gated, reversed problems included
 *   exactly one given       SOSVO_ERR_ARG
 * For query i of a FORWARD problem (p < n_forward) let k1 < k2 be the two smallest keys (hamming << 20 | j) over the
 * admissible trains, d1 = k1 >> 20, d2 = k2 >> 20.  All distances are integers, and so is the rule:
 *   keep(i)  <=>  64 * d1 < ratio_64ths * d2                 (ratio_64ths 1 .. 63; 48 is d1 < d2 * 0.75 for all integers)
 *   keys[p*q_stride + i]   = k1 if keep(i) and d1 <= max_distance, else SOSVO_KEY_NONE   (the cap acts after the rule)
 *   rivals[p*q_stride + i] = k2, or SOSVO_KEY_NONE if fewer than two trains are admissible
 * Two trains at the same distance never pass (not even at distance 0); ties between trains are resolved by the key order
 * (lowest train index first).  NO RUNNER-UP (fewer than two admissible trains): the plain form drops the match, as the
 * reference's len(m) == 2 does; the gated form KEEPS it -- a partner that is alone inside the geometric gate is unique by
 * construction.  The form decides, not the gate values: the gated form with both gate sides disabled still keeps a lone
 * train, and that is the one place where it differs from the plain form.
 * REVERSED problems (p >= n_forward) only answer "did train j choose i back" for sosvo_cross_check_matches and get no
 * rule: their keys are those of sosvo_match_hamming(k = 1) (plain) or sosvo_match_hamming_gated (gated), bit for bit, and
 * their rows of rivals are unspecified.  After the cross-check a match thus survives iff it passes the rule AND is mutual.
 * keys and rivals are [nprob, q_stride] u32 and BOTH required: rivals is the second merge word of the train-range split.
 * Rows i >= nq[qs] are unspecified.  The results do not depend on how the train range is split.  Wherever a key is not
 * SOSVO_KEY_NONE it is the key of the search of the same form without the rule. */
int32_t sosvo_match_hamming_ratio(sosvo_ctx* ctx, const uint8_t* q_desc, const uint8_t* t_desc, const float* q_pos,
                                  const float* t_pos, const int32_t* nq, const int32_t* nt, const int32_t* q_slot,
                                  const int32_t* t_slot, int32_t nprob, int32_t n_forward, int32_t q_stride, int32_t t_stride,
                                  double min_dv, double max_du, int32_t max_distance, int32_t ratio_64ths,
                                  uint32_t* keys, uint32_t* rivals);

/* Float descriptors (SIFT / SURF / KAZE ...; feature_detection_method "SIFT" / "SURF" makes FeatureMatcher build
 * cv2.BFMatcher() with its default NORM_L2, omnistereo/camera_models.py:394-396): brute-force L2 matching.
 * q_desc [nprob, q_stride, dim] f32, t_desc [nprob, t_stride, dim] f32, dim <= 128, finite values.  distance = sqrt of the
 * float32 sum of squared differences, four terms per step in index order (OpenCV's scalar normL2Sqr_).
 *   keys[(p*q_stride + i)*k + r] = (bits of the float32 distance << 32) | train index of the r-th neighbour (r < k,
 *   k = 1 or 2; smallest distance, first train index on ties), all ones if absent.
 * The reference's FLANN matcher (camera_models.py:384-393: KD-trees for float, LSH for binary descriptors, randomised,
 * approximate) has no counterpart: matcher_type "FLANN" is served by the exact searches (sosvo_match_hamming / this). */
int32_t sosvo_match_l2(sosvo_ctx* ctx, const float* q_desc, const float* t_desc, const int32_t* nq, const int32_t* nt,
                       int32_t nprob, int32_t q_stride, int32_t t_stride, int32_t dim, int32_t k, uint64_t* keys);

/* Radius match: cv2.BFMatcher.radiusMatch(query, train, maxDistance) as called from FeatureMatcher.match when
 * use_radius_match is set (omnistereo/camera_models.py:412-415).  For each query row i < nq[qs] ALL train rows j
 * with hamming(q_i, t_j) <= max_distance, as packed keys in ascending order (distance, then train index):
 *   keys[(p*q_stride + i)*cap + r], r < min(counts, cap); the rest SOSVO_KEY_NONE
 *   counts[p*q_stride + i] = number of train rows within the radius (when it exceeds cap, the cap smallest
 *   keys are the ones kept).  cap <= 512.  Blocks / slots as in sosvo_match_hamming.                      */
int32_t sosvo_match_radius(sosvo_ctx* ctx, const uint8_t* q_desc, const uint8_t* t_desc, const int32_t* nq,
                           const int32_t* nt, const int32_t* q_slot, const int32_t* t_slot, int32_t nprob,
                           int32_t q_stride, int32_t t_stride, int32_t max_distance, int32_t cap,
                           uint32_t* keys, int32_t* counts);

/* Mutual-consistency filter: cv2.BFMatcher(normType=cv2.NORM_HAMMING, crossCheck=True), the matcher the reference
 * carries commented out at omnistereo/camera_models.py:401.  keys_fwd [nprob, q_stride] are the keys of
 * sosvo_match_hamming(k = 1) for the problems (nq, nt, q_slot, t_slot); keys_rev [nprob, t_stride] those of the same call
 * with query and train (descriptors, counts, slots and strides) swapped, so keys_rev[p*t_stride + j] names the query
 * closest to train j, lowest query index on ties.  For each query row i < nq[qs]:
 *   keys_out[p*q_stride + i] = keys_fwd[p*q_stride + i]  if its train j chose i back: (keys_rev[p*t_stride + j] & IDX_MASK) == i
 *                            = SOSVO_KEY_NONE            otherwise (and where keys_fwd is SOSVO_KEY_NONE)
 *   n_kept[p] = number of kept matches (n_kept may be NULL).
 * Rows i >= nq[qs] are not written.  keys_out may be keys_fwd.  sosvo_sort_matches puts the kept matches first, in the
 * order sorted() gives them; the assemble stages take len(matches) as the number of keys that are not SOSVO_KEY_NONE.
 * Defined for 1-NN Hamming keys only (OpenCV refuses crossCheck with k > 1).  Counts / slots as in sosvo_match_hamming. */
int32_t sosvo_cross_check_matches(sosvo_ctx* ctx, const uint32_t* keys_fwd, const uint32_t* keys_rev, const int32_t* nq,
                                  const int32_t* nt, const int32_t* q_slot, const int32_t* t_slot, int32_t nprob,
                                  int32_t q_stride, int32_t t_stride, uint32_t* keys_out, int32_t* n_kept);

/* Stable sort of each problem's 1-NN matches by distance, the `sorted(matches,
 * key=distance)` of omnistereo/camera_models.py:444.  Input keys as written by
 * sosvo_match_hamming with k = 1.  Output, for rank r < nq[qs]:
 *   order[p*q_stride + r] = query index of the r-th match (ties keep query order).
 * Queries whose key is SOSVO_KEY_NONE (empty train set) sort last.  q_stride <= 16384.    */
int32_t sosvo_sort_matches(sosvo_ctx* ctx, const uint32_t* keys, const int32_t* nq,
                           const int32_t* q_slot, int32_t nprob, int32_t q_stride, int32_t* order);

/* ---- K8 / K10: 3D-2D absolute-pose RANSAC ------------------------------------------------
 * Replaces pyopengv.absolute_pose_noncentral_ransac (omnistereo/pose_est_tools.py:785) and
 * pyopengv.absolute_pose_ransac (:915).  Batched: problem b owns rows [b*stride, b*stride+n[b]).
 *   f   [nprob*stride, 3] f64  unit bearings of the CURRENT frame, in their camera's frame
 *   p   [nprob*stride, 3] f64  3-D points of the REFERENCE frame (frame [C], model units)
 *   cam [nprob*stride]    i32  camera index per correspondence, or NULL for the central case
 *   cam_off [ncam,3], cam_rot [ncam,3,3] f64 row-major: camera position / rotation wrt the
 *       viewpoint (TrackerStereoSE3.bootstrap_tracker, pose_est_tools.py:852-859); shared by the batch
 *   flags: SOSVO_FLAG_CAM_ROT_IDENTITY promises cam_rot are identities (skips a mat-vec; results
 *       are bit-identical for finite data)
 *   thr: inlier iff 1 - f . f_hat < thr (pose_est_tools.py:675-676: 1 - cos 5 deg)
 *   max_iter hypotheses are drawn by a counter-based sampler from (seed + b, iteration); with
 *   adaptive != 0 the sequential early stop of OpenGV's sac::Ransac (probability 0.99, sample
 *   size 4) is replayed over them, so the result equals a sequential run on the same samples.
 * Outputs per problem: T_out [nprob,3,4] = [R|t] (pose of the current viewpoint in the reference
 * frame: X_ref = R x + t), inlier_mask [nprob*stride] u8, inlier_idx [nprob*stride] i32 ascending
 * (first n_inliers[b] entries), n_inliers [nprob], info [nprob,4] = {best iteration (-1: none),
 * iterations drawn, status (0 ok / 1 no model -> T = identity), number of valid hypotheses}.
 * hyp_counts: optional [nprob,max_iter] i32, receives each hypothesis' inlier count (-1: the
 * minimal solve failed); NULL to keep them in the context workspace.                         */
#define SOSVO_FLAG_CAM_ROT_IDENTITY 1
/* central problems (cam == NULL): hypotheses from EPnP on 6-point samples, as OpenGV's absolute_pose_ransac does for
 * algorithm "EPNP" (the RGB-D tracker's choice, pose_est_tools.py:697, :915), instead of Kneip P3P + a 4th point;
 * the adaptive stop then uses w^6. */
#define SOSVO_FLAG_EPNP 2
/* hypotheses from the GENERALISED P3P: four distinct correspondences out of ALL cameras, the generalised three-point
 * problem on the first three (up to 8 poses), the fourth picks one -- what OpenGV's non-central problem does ("will
 * ALWAYS use GP3P", pose_est_tools.py:696, :785).  Without the flag the three solve points of a sample come from ONE
 * camera (central Kneip P3P moved to the body frame; BASELINE config 2's "P3P RANSAC").  Also valid for central
 * problems (then a P3P that only returns configurations in front of the camera). */
#define SOSVO_FLAG_GP3P 4
/* central problems: "TWOPT" (pose_est_tools.py:95-107) -- 2-point samples, the translation of a camera whose rotation is
 * known (the identity, as pyopengv's binding leaves OpenGV's rotation prior); the adaptive stop then uses w^2. */
#define SOSVO_FLAG_TWOPT 8
int32_t sosvo_ransac_abs_pose(sosvo_ctx* ctx, const double* f, const double* p, const int32_t* cam,
                              const double* cam_off, const double* cam_rot, int32_t ncam, int32_t flags,
                              const int32_t* n, int32_t nprob, int32_t stride, double thr,
                              int32_t max_iter, int32_t adaptive, uint64_t seed, double* T_out,
                              uint8_t* inlier_mask, int32_t* inlier_idx, int32_t* n_inliers,
                              int32_t* info, int32_t* hyp_counts);
/* As sosvo_ransac_abs_pose with ONE SEED PER PROBLEM: problem b samples from (seeds[b], iteration), seeds [nprob] u64
 * (device).  The problems of a call then need not be consecutive frames of one sequence (the multi-sequence entry points
 * below: lane s is at frame t_s and tracks with seed t_s - 1).  seeds[b] = seed + b gives sosvo_ransac_abs_pose(seed)
 * exactly; everything but the sampler's seed (solvers, scoring, adaptive stop, outputs) is shared.                 */
int32_t sosvo_ransac_abs_pose_seeds(sosvo_ctx* ctx, const double* f, const double* p, const int32_t* cam,
                                    const double* cam_off, const double* cam_rot, int32_t ncam, int32_t flags,
                                    const int32_t* n, int32_t nprob, int32_t stride, double thr,
                                    int32_t max_iter, int32_t adaptive, const uint64_t* seeds, double* T_out,
                                    uint8_t* inlier_mask, int32_t* inlier_idx, int32_t* n_inliers,
                                    int32_t* info, int32_t* hyp_counts);

/* ---- K9: non-linear refinement --------------------------------------------------------------
 * Replaces pyopengv.absolute_pose_noncentral_optimize_nonlinear (pose_est_tools.py:830) and
 * absolute_pose_optimize_nonlinear (:937): Levenberg-Marquardt on (t, Cayley(R)), residual
 * 1 - f . f_hat per correspondence, analytic Jacobian (OpenGV differentiates numerically).  Same layout as the
 * RANSAC call;
 * idx/m (both or neither): the first m[b] entries of idx[b*stride ...] select the correspondences
 * (e.g. inlier_idx / n_inliers of sosvo_ransac_abs_pose); NULL = all n[b].
 * T_io [nprob,3,4] in: start pose, out: refined pose.  cost_out [nprob] f64 and iters_out
 * [nprob] i32 are optional.                                                                      */
int32_t sosvo_refine_abs_pose(sosvo_ctx* ctx, const double* f, const double* p, const int32_t* cam,
                              const double* cam_off, const double* cam_rot, int32_t ncam,
                              const int32_t* n, int32_t nprob, int32_t stride, const int32_t* idx,
                              const int32_t* m, int32_t max_lm_iter, double* T_io, double* cost_out,
                              int32_t* iters_out);

/* ---- 2D-2D relative-pose RANSAC ------------------------------------------------
 * Replaces pyopengv.relative_pose_ransac(b1, b2, algorithm, threshold, max_iterations) as called by
 * pose_relative_ransac_2D_to_2D (omnistereo/pose_est_tools.py:54-90, call at :78).
 * f1, f2 [nprob*stride,3] f64: unit bearings of the SAME features seen from viewpoints 1 and 2; n [nprob].
 * Score of a correspondence under (R, t) -- the reference's own restatement, pose_est_tools.py:150-203: X = the midpoint
 * triangulation (OpenGV triangulate2) in frame 1, score = (1 - f1 . X/|X|) + (1 - f2 . x2/|x2|), x2 = R^T (X - t); inlier
 * iff score < thr.  algorithm selects the minimal solver (sample size incl. the disambiguation points in brackets):
 * SOSVO_REL_FIVEPT (5 + 3; Nister's five-point algorithm, the reference's default "STEWENIUS" and "NISTER"),
 * SOSVO_REL_SEVENPT (7 + 2), SOSVO_REL_EIGHTPT (8).  Among all decompositions of all essential matrices of a sample the
 * (R, t) with the smallest summed score over the sample becomes the hypothesis.  Outputs as sosvo_ransac_abs_pose: T_out [nprob,3,4] = [R | t], the pose of viewpoint 2 in
 * frame 1 (X1 = R X2 + t), |t| = 1 (the scale of a 2D-2D motion is unobservable). */
#define SOSVO_REL_FIVEPT 5
#define SOSVO_REL_SEVENPT 7
#define SOSVO_REL_EIGHTPT 8
int32_t sosvo_ransac_rel_pose(sosvo_ctx* ctx, const double* f1, const double* f2, const int32_t* n, int32_t nprob,
                              int32_t stride, int32_t algorithm, double thr, int32_t max_iter, int32_t adaptive,
                              uint64_t seed, double* T_out, uint8_t* inlier_mask, int32_t* inlier_idx,
                              int32_t* n_inliers, int32_t* info, int32_t* hyp_counts);

/* ---- geometry: a7-a10, a12 -------------------------------------------------------------------
 * Elementwise restatements of the reference's numpy geometry (FP64; values agree with the
 * reference to rel-tol 1e-12, the transcendental functions come from the device math library).
 *
 * sosvo_pano_to_bearing: uv [n,2] pano pixel -> az, el, bearing [n,3] (any output may be NULL).
 *   Panorama.get_direction_angles_from_pixel_pano (omnistereo/panorama.py:650, closed form :635,:616),
 *   GUM.get_3D_point_from_angles_wrt_focus (gum.py:2564) -> map_angles_to_unit_sphere
 *   (camera_models.py:1031).  NaN outside [0,cols) x [0,rows).
 * sosvo_triangulate_midpoint: OmniStereoModel.get_triangulated_point_from_direction_angles
 *   (camera_models.py:3323, use_midpoint_triangulation=True) -> get_triangulated_midpoint (:2420)
 *   -> triangulate_for_skew_rays (:2481).  F_top_host / F_bot_host: HOST pointers to 3 doubles.
 * sosvo_triangulate2: pyopengv.triangulation_triangulate2(b1, b2, t12, R12) (pose_est_tools.py:359, :163):
 *   OpenGV's closed-form midpoint, g = R12 b2, [[b1.b1, -b1.g], [b1.g, -g.g]] lambda = (t12.b1, t12.g),
 *   X = (lambda0 b1 + t12 + lambda1 g) / 2 in frame 1.  b1, b2, X [n,3] device; t12 (3), R12 (9, row-major) HOST.
 * sosvo_range_filter: filter_panoramic_points_due_to_range (camera_models.py:3299) as called with
 *   homogeneous rows at pose_est_tools.py:372 (norm includes the trailing 1); limit <= 0 disables.
 * sosvo_rgbd_backproject: RGBDCamModel.get_XYZ (camera_models.py:835) + get_depth_Z (:781) at
 *   integer pixels + get_normalized_points (:203).  depth [rows,cols] f32; zeros -> NaN.        */
int32_t sosvo_pano_to_bearing(sosvo_ctx* ctx, const double* uv, int32_t n, double cols, double rows,
                              double pixel_size, double cyl_height_max, double* az, double* el,
                              double* bearing);
int32_t sosvo_triangulate_midpoint(sosvo_ctx* ctx, const double* az_top, const double* el_top,
                                   const double* az_bot, const double* el_bot, int32_t n,
                                   const double* F_top_host, const double* F_bot_host, double* X);
int32_t sosvo_triangulate2(sosvo_ctx* ctx, const double* b1, const double* b2, int32_t n, const double* t12_host,
                           const double* R12_host, double* X);
int32_t sosvo_range_filter(sosvo_ctx* ctx, const double* X, int32_t n, double min_range,
                           double max_range, uint8_t* ok);
int32_t sosvo_rgbd_backproject(sosvo_ctx* ctx, const float* depth, int32_t rows, int32_t cols,
                               const int32_t* u, const int32_t* v, int32_t n, double fx, double fy,
                               double cx, double cy, double focal_length_m, int32_t depth_is_Z,
                               double* xyz, double* bearing);

/* Constants of one calibrated omnistereo rig as the hot path needs them (HOST struct, passed by
 * pointer and copied into kernel arguments).  pano_* = {cols, rows, pixel_size, cyl_height_max}
 * of Panorama (panorama.py:142-172); F_* = mirror foci wrt [C]; ranges in model units
 * (pose_est_tools.py:306-308); gates of pose_est_tools.py:298-304 and :866; pct_good_matches of
 * FeatureMatcher (camera_models.py:379).                                                         */
typedef struct sosvo_rig {
  double pano_top[4];
  double pano_bot[4];
  double F_top[3];
  double F_bot[3];
  double min_range;        /* <= 0 disables */
  double max_range;        /* <= 0 disables */
  double stereo_min_disp;  /* v_top - v_bot >= this, < 0 disables (common_cv.py:182) */
  double stereo_max_hdiff; /* |u_top - u_bot| <= this, <= 0 disables (common_cv.py:177) */
  double f2f_max_hdiff;    /* frame-to-frame |du| gate, <= 0 disables (< 0 skips it, pose_est_tools.py:245; 0 passes all) */
  double pct_good_matches; /* 1.0 */
} sosvo_rig;

/* ---- stereo assemble: a6 + a7..a11 fused ------------------------------------------------------
 * Replaces OmniStereoModel.match_features_panoramic_top_bottom (camera_models.py:3027-3101) after
 * the per-bucket matcher call, and StereoPanoramicFrame.establish_stereo_correspondences
 * (pose_est_tools.py:339-397).  Problem p = frame*nmask + mask owns rows [p*cap, p*cap + n_*[p]) of
 * kp_* [.,2] f32 / desc_* [.,32] u8; keys/order [nframes*nmask, cap] come from sosvo_match_hamming
 * (query = bottom, train = top, k = 1) and sosvo_sort_matches.  Per frame, candidates are visited
 * in bucket order then rank order (empty buckets skipped), gated (|du|, dv), lifted to angles and
 * bearings, triangulated, range-filtered, and the survivors are written in that order:
 * m_top/m_bot [nframes,out_cap,2] f32, d_top/d_bot [nframes,out_cap,32] u8, X (frame [C]),
 * b_top/b_bot [nframes,out_cap,3] f64, M [nframes] i32 (count), n_cand [nframes] (optional:
 * candidates before the gates).  This is the PanoramicCorrespondences contract
 * (camera_models.py:291-362) in structure-of-arrays form.  A frame with more survivors than out_cap keeps the first
 * out_cap in that order (M = out_cap): what the reference's arrays hold, cut after out_cap rows.  */
int32_t sosvo_stereo_assemble(sosvo_ctx* ctx, const sosvo_rig* rig_host, const float* kp_top,
                              const float* kp_bot, const uint8_t* desc_top, const uint8_t* desc_bot,
                              const int32_t* n_top, const int32_t* n_bot, const uint32_t* keys,
                              const int32_t* order, int32_t nframes, int32_t nmask, int32_t cap,
                              int32_t out_cap, float* m_top, float* m_bot, uint8_t* d_top,
                              uint8_t* d_bot, double* X, double* b_top, double* b_bot, int32_t* M,
                              int32_t* n_cand);

/* ---- frame-to-frame assemble: a13 + the stacking of a14 ---------------------------------------
 * Replaces match_features_frame_to_frame (pose_est_tools.py:211-269) after the matcher call and
 * the correspondence stacking of TrackerStereoSE3.track_frame (:752-778).  Pair pr tracks frame
 * cur_frame[pr] against (key)frame ref_frame[pr]; keys_top, order_top, keys_bot, order_bot
 * [npairs, frame_cap] come from
 * matching query = current, train = reference per view (use q_slot = cur_frame, t_slot =
 * ref_frame).  Output rows [pr*corr_cap ...): top-view correspondences first, then bottom view,
 * each in rank order after the |du| gate: f = bearing of the current frame, p = 3-D point of the
 * reference frame, cam = 0/1, corr_q / corr_t = indices into the two frames, n [npairs] = count,
 * n_topview [npairs] (optional) = how many of them are top-view.                                 */
int32_t sosvo_f2f_assemble(sosvo_ctx* ctx, const sosvo_rig* rig_host, const float* m_top,
                           const float* m_bot, const double* X, const double* b_top,
                           const double* b_bot, const int32_t* M, int32_t frame_cap,
                           const int32_t* ref_frame, const int32_t* cur_frame, const uint32_t* keys_top,
                           const int32_t* order_top, const uint32_t* keys_bot, const int32_t* order_bot,
                           int32_t npairs, int32_t corr_cap, double* f, double* p, int32_t* cam,
                           int32_t* corr_q, int32_t* corr_t, int32_t* n, int32_t* n_topview);

/* The twin of sosvo_f2f_assemble for TRACKED points (sosvo_track_lk in place of the matcher): pair pr tracked the points
 * m_top / m_bot [.., frame_cap, 2] of (key)frame ref_frame[pr] into its current frame; trk_top, trk_bot [npairs, frame_cap, 2]
 * f32 are the tracked pixels and st_top, st_bot [npairs, frame_cap] u8 their status, rows k < min(M[ref_frame[pr]], frame_cap).
 * Output rows [pr*corr_cap ...) in the layout sosvo_ransac_abs_pose reads: top-view correspondences first, then bottom view,
 * each in POINT order; a point is kept when its status is not 0 and |u_tracked - u_reference| <= f2f_max_hdiff (the gate is
 * disabled as in sosvo_f2f_assemble).  f = the bearing of the tracked pixel through the pixel-to-bearing code of
 * sosvo_stereo_assemble for that view (pano_top / pano_bot of the rig), p = the 3-D point X of the reference frame,
 * cam = 0/1, corr_t = the point's index in the reference frame, corr_q = -1 (the current frame has no keypoint index),
 * n [npairs] = count (at most corr_cap: the first corr_cap are kept), n_topview [npairs] (optional).                   */
int32_t sosvo_f2f_assemble_tracked(sosvo_ctx* ctx, const sosvo_rig* rig_host, const float* m_top, const float* m_bot,
                                   const double* X, const int32_t* M, int32_t frame_cap, const int32_t* ref_frame,
                                   const float* trk_top, const float* trk_bot, const uint8_t* st_top, const uint8_t* st_bot,
                                   int32_t npairs, int32_t corr_cap, double* f, double* p, int32_t* cam, int32_t* corr_q,
                                   int32_t* corr_t, int32_t* n, int32_t* n_topview);

/* The two assembles with the CYCLIC |du| gate: a panorama is a full circle, column W is column 0
 * again, W = pano_top[0] / pano_bot[0] of the rig for the view.  With d = |u_a - u_b| computed in double from the float32
 * values, a pair passes iff d <= f2f_max_hdiff or W - d <= f2f_max_hdiff; the gate's switch is the plain one's (off for
 * f2f_max_hdiff <= 0).  Both comparisons are exact: differences of float32 coordinates below 16384, and W - d, are
 * representable in double.  Arguments, outputs and order exactly as in sosvo_f2f_assemble / sosvo_f2f_assemble_tracked; the
 * two periods must be positive integers (up to 16384), otherwise SOSVO_ERR_ARG.                                          */
int32_t sosvo_f2f_assemble_cyclic(sosvo_ctx* ctx, const sosvo_rig* rig_host, const float* m_top, const float* m_bot,
                                  const double* X, const double* b_top, const double* b_bot, const int32_t* M,
                                  int32_t frame_cap, const int32_t* ref_frame, const int32_t* cur_frame,
                                  const uint32_t* keys_top, const int32_t* order_top, const uint32_t* keys_bot,
                                  const int32_t* order_bot, int32_t npairs, int32_t corr_cap, double* f, double* p,
                                  int32_t* cam, int32_t* corr_q, int32_t* corr_t, int32_t* n, int32_t* n_topview);
int32_t sosvo_f2f_assemble_tracked_cyclic(sosvo_ctx* ctx, const sosvo_rig* rig_host, const float* m_top, const float* m_bot,
                                          const double* X, const int32_t* M, int32_t frame_cap, const int32_t* ref_frame,
                                          const float* trk_top, const float* trk_bot, const uint8_t* st_top,
                                          const uint8_t* st_bot, int32_t npairs, int32_t corr_cap, double* f, double* p,
                                          int32_t* cam, int32_t* corr_q, int32_t* corr_t, int32_t* n, int32_t* n_topview);

/* ---- RGB-D (perspective camera) variant: a12 + a15 glue ----------------------------------------
 * Constants of one RGB-D camera (HOST struct): RGBDCamModel (omnistereo/camera_models.py:756-779) and the
 * RGBDFrame ranges (pose_est_tools.py:428-430, in the depth map's units).                           */
typedef struct sosvo_rgbd_cam {
  double fx, fy, cx, cy;
  double focal_length_m;   /* only used when depth is radial (depth_is_Z == 0, camera_models.py:781-799) */
  int32_t depth_is_Z;      /* 1: the depth map holds Z values */
  int32_t reserved;
  double min_range;        /* keep min_range <= |Z| <= max_range; <= 0 disables (pose_est_tools.py:570-592) */
  double max_range;
} sosvo_rgbd_cam;

/* sosvo_rgbd_assemble: RGBDFrame.establish_keypoints after detection (pose_est_tools.py:609-623) for nframes
 * frames: depth at the keypoints' integer pixels -> XYZ (get_XYZ), keypoints with zero depth (NaN) or out of
 * range dropped, bearings = normalised XYZ, survivors written in keypoint order.
 *   kp [nframes, cap, 2] f32, desc [nframes, cap, 32] u8, n [nframes] i32, depth [nframes, rows, cols] f32
 *   -> m [nframes, out_cap, 2] f32, d [nframes, out_cap, 32] u8, X, b [nframes, out_cap, 3] f64, M [nframes] i32
 * sosvo_f2f_assemble_central: TrackerRGBDSE3.track_frame steps 1-2 (pose_est_tools.py:896-913) for npairs pairs:
 *   keys / order [npairs, frame_cap] from sosvo_match_hamming (query = current frame's d, train = reference
 *   frame's d, k = 1) + sosvo_sort_matches; the first pct_good_matches * nq matches (:225), |du| <= max_hdiff
 *   (<= 0 disables, :245-247) -> f (bearings of the current frame), p (points of the reference frame)
 *   [npairs, corr_cap, 3] f64, corr_q / corr_t [npairs, corr_cap] i32 (indices into the frames), n [npairs].
 *   Feed f, p, n to sosvo_ransac_abs_pose / sosvo_refine_abs_pose with cam = NULL (central, :915, :937).   */
int32_t sosvo_rgbd_assemble(sosvo_ctx* ctx, const sosvo_rgbd_cam* cam_host, const float* kp, const uint8_t* desc,
                            const int32_t* n, const float* depth, int32_t nframes, int32_t rows, int32_t cols,
                            int32_t cap, int32_t out_cap, float* m, uint8_t* d, double* X, double* b, int32_t* M);
int32_t sosvo_f2f_assemble_central(sosvo_ctx* ctx, double pct_good_matches, double max_hdiff, const float* m,
                                   const double* X, const double* b, const int32_t* M, int32_t frame_cap,
                                   const int32_t* ref_frame, const int32_t* cur_frame, const uint32_t* keys,
                                   const int32_t* order, int32_t npairs, int32_t corr_cap, double* f, double* p,
                                   int32_t* corr_q, int32_t* corr_t, int32_t* n);

/* ---- keypoint detectors of the batch and sequence entry points ------------------------------------
 * sosvo_batch_cfg.detector, and bits 8-9 of sosvo_rgbd_batch_cfg.flags (SOSVO_RGBD_DETECTOR(d)), select the
 * feature_detection_method (pose_est_tools.py:684, :477-516).  The RGB-D detector bits never reach the RANSAC flags. */
enum sosvo_detector { SOSVO_DETECTOR_GFT = 0, SOSVO_DETECTOR_ORB = 1, SOSVO_DETECTOR_FAST = 2, SOSVO_DETECTOR_AGAST = 3 };
#define SOSVO_RGBD_DETECTOR_SHIFT 8
#define SOSVO_RGBD_DETECTOR_MASK (3 << SOSVO_RGBD_DETECTOR_SHIFT)
#define SOSVO_RGBD_DETECTOR(d) ((d) << SOSVO_RGBD_DETECTOR_SHIFT)
#define SOSVO_RGBD_DETECTOR_OF(flags) (((flags) & SOSVO_RGBD_DETECTOR_MASK) >> SOSVO_RGBD_DETECTOR_SHIFT)

/* ---- mutual-consistency (cross-check) matching in the batch and sequence entry points --------------------
 * The reference has two matcher objects, and each may be built with crossCheck=True (camera_models.py:401):
 *   SOSVO_FLAG_CROSS_CHECK_STEREO  feature_matcher_for_static_stereo: top / bottom matching per azimuthal bucket
 *   SOSVO_FLAG_CROSS_CHECK_F2F     feature_matcher_for_motion: frame-to-frame matching per view (RGB-D: the one matcher)
 * Both are honoured in sosvo_batch_cfg.ransac_flags, ..._F2F in sosvo_rgbd_batch_cfg.flags; ..._STEREO in an RGB-D
 * configuration is SOSVO_ERR_ARG (and a workspace size of 0).  With a bit set, the forward and the role-swapped problems
 * of a matching step run as ONE sosvo_match_hamming launch over a slot table, sosvo_cross_check_matches filters the
 * forward keys, and the sort / assemble stages follow as always: int(pct_good_matches * len(matches)) then counts the
 * kept matches.  The workspaces grow by the reverse keys and the slot tables only when a bit is set; with both clear
 * sizes, launches and results are unchanged.  The bits never reach the RANSAC flags.  A matching launch holds at most 65535
 * problems (sosvo_match_hamming), forward and reverse together: frames x nmask <= 32767 per front-end call with ..._STEREO,
 * pairs <= 32767 per tracking call with ..._F2F (n_pairs <= 8192 anyway). */
#define SOSVO_FLAG_CROSS_CHECK_STEREO 0x1000
#define SOSVO_FLAG_CROSS_CHECK_F2F 0x2000

/* ---- gated matching in the batch and sequence entry points (sosvo_match_hamming_gated) ----------------------
 *   SOSVO_FLAG_GATED_STEREO  static stereo: each bottom keypoint takes its nearest top keypoint of the bucket among those
 *                            that pass the rig's stereo_min_disp / stereo_max_hdiff gate
 *   SOSVO_FLAG_GATED_F2F     frame to frame, per view: the nearest keypoint of the reference frame within f2f_max_hdiff
 *                            columns; the gate is disabled exactly when the assemble stage's is (f2f_max_hdiff <= 0 in
 *                            sosvo_rig and in sosvo_rgbd_batch_cfg: below 0 the stage skips its gate, at 0 the gate
 *                            passes every pair)
 *   SOSVO_GATED_MAX_DIST(d)  bits 16-24: 0 = no cap; 1 .. 256: a match whose distance exceeds d is no match (a larger
 *                            field value is SOSVO_ERR_ARG, from sosvo_match_hamming_gated); ignored without a GATED bit
 * Honoured in sosvo_batch_cfg.ransac_flags; ..._F2F and the distance field in sosvo_rgbd_batch_cfg.flags, ..._STEREO there
 * is SOSVO_ERR_ARG (and a workspace size of 0).  A query without an admissible partner has the key SOSVO_KEY_NONE; sort
 * and assemble treat it as after the cross-check filter, and the assemble gates stay (they now pass every match they see).
 * Together with SOSVO_FLAG_CROSS_CHECK_*: the role-swapped problems run under the same gate in the same launch ("mutual
 * under the gate"; the gate is symmetric in the pair).  The bits never reach the RANSAC flags; the struct layouts and,
 * with the bits clear, workspace sizes, launches and results are unchanged -- the gated search needs no workspace. */
#define SOSVO_FLAG_GATED_STEREO 0x4000
#define SOSVO_FLAG_GATED_F2F 0x8000
#define SOSVO_GATED_MAX_DIST_SHIFT 16
#define SOSVO_GATED_MAX_DIST_MASK (0x1FF << SOSVO_GATED_MAX_DIST_SHIFT)
#define SOSVO_GATED_MAX_DIST(d) ((d) << SOSVO_GATED_MAX_DIST_SHIFT)
#define SOSVO_GATED_MAX_DIST_OF(flags) (((flags) & SOSVO_GATED_MAX_DIST_MASK) >> SOSVO_GATED_MAX_DIST_SHIFT)

/* ---- the ratio rule in the batch and sequence entry points (sosvo_match_hamming_ratio) -----------------------
 *   SOSVO_FLAG_RATIO_STEREO  static stereo: a bottom keypoint's match is kept only if 64 * d1 < r * d2 against the runner-up
 *   SOSVO_FLAG_RATIO_F2F     frame to frame, per view: likewise
 *   SOSVO_RATIO_64THS(r)     bits 25-30: the ratio r in 64ths, 1 .. 63 (48 = the reference's 0.75); a switch bit with the
 *                            field 0 is SOSVO_ERR_ARG (and a workspace size of 0); ignored without a RATIO bit
 * Honoured in sosvo_batch_cfg.ransac_flags; ..._F2F and the field in sosvo_rgbd_batch_cfg.flags, ..._STEREO there is
 * SOSVO_ERR_ARG (and a workspace size of 0).  Without SOSVO_FLAG_GATED_* of the same step the plain form runs (a query with
 * a single train has no match); with it the gated form: the runner-up is sought among the admissible trains, a partner
 * alone inside the gate is kept, and the cap acts after the rule.  Together with SOSVO_FLAG_CROSS_CHECK_*: the
 * role-swapped problems get no rule, so a match survives iff it passes the rule AND is mutual; one launch as before.
 * A dropped match has the key SOSVO_KEY_NONE; sort and assemble treat it as after the cross-check filter.  The bits never
 * reach the RANSAC flags; the struct layouts and, with the switch bits clear, workspace sizes, launches and results are
 * unchanged.  With a switch set the workspace grows by that step's rivals (one u32 per key of the step). */
#define SOSVO_FLAG_RATIO_STEREO 0x10
#define SOSVO_FLAG_RATIO_F2F 0x20
#define SOSVO_RATIO_64THS_SHIFT 25
#define SOSVO_RATIO_64THS_MASK (0x3F << SOSVO_RATIO_64THS_SHIFT)
#define SOSVO_RATIO_64THS(r) ((r) << SOSVO_RATIO_64THS_SHIFT)
#define SOSVO_RATIO_64THS_OF(flags) (((flags) & SOSVO_RATIO_64THS_MASK) >> SOSVO_RATIO_64THS_SHIFT)

/* ---- sub-pixel keypoint refinement in the batch and sequence entry points (sosvo_refine_subpix) --------------
 *   SOSVO_FLAG_SUBPIX        refine every keypoint after the descriptor stage and before the static-stereo matching
 *   SOSVO_SUBPIX_HALF(h)     bits 10-11: the window half-size h = 2 .. 5, stored as h - 2; ignored without the switch bit
 * max_iter is 10 and eps 0.01 here.  Honoured in sosvo_batch_cfg.ransac_flags for every detector (ORB: on kp_xy; kp4 keeps
 * the detector's positions).  Descriptors stay those of the unrefined positions, bit for bit; the stereo gates, the gated
 * search, bearings, triangulation, the frame records' m_top / m_bot and everything after them see the refined positions.
 * In sosvo_rgbd_batch_cfg.flags the switch is SOSVO_ERR_ARG (and a workspace size of 0): depth is read at integer pixels.
 * The bits never reach the RANSAC flags; the struct layouts and, with the switch clear, workspace sizes, launches and
 * results are unchanged -- the stage needs no workspace. */
#define SOSVO_FLAG_SUBPIX 0x40
/* ---- Lucas-Kanade tracking in the batch and sequence entry points (sosvo_track_lk in place of the frame-to-frame matcher) ----
 *   SOSVO_FLAG_LK_F2F        the tracking step follows the reference frame's stereo points m_top / m_bot into the current
 *                            frame's gray panoramas (one sosvo_track_lk launch of 2 B problems, top views first) and stacks
 *                            them with sosvo_f2f_assemble_tracked; the two match / sort pairs and sosvo_f2f_assemble do not
 *                            run.  RANSAC, the refinement and the [B, 16] records follow as always.
 * Honoured in sosvo_batch_cfg.ransac_flags; in sosvo_rgbd_batch_cfg.flags it is SOSVO_ERR_ARG (and a workspace size of 0).
 * Together with SOSVO_FLAG_CROSS_CHECK_F2F, SOSVO_FLAG_GATED_F2F or SOSVO_FLAG_RATIO_F2F it is SOSVO_ERR_ARG (size 0) as well:
 * they act on a matcher that no longer runs.  The ..._STEREO bits and SOSVO_FLAG_SUBPIX combine freely with it.  The bit never
 * reaches the RANSAC flags; the struct layouts and, with the bit clear, workspace sizes, launches and results are unchanged.
 *
 * The tracker's six settings do not fit the flags: they belong to the CONTEXT (sosvo_set_lk_options).  A new context has the
 * defaults SOSVO_LK_OPTIONS_DEFAULT: half 10, levels 3, max_iter 30, eps 0.01, min_eig 1e-4, no check.  fb_max <= 0: no
 * forward-backward check.  The ranges are sosvo_track_lk's (and finite values); a refused call -- a value out of range, or a
 * NULL pointer, as everywhere in this ABI -- is SOSVO_ERR_ARG and leaves the previous settings.
 * Unlike the hints they change results: sosvo_frame_pair_batch_streams* hands them to its internal contexts at every call.
 *
 * With the bit set the frame store also keeps every frame's gray panoramas and their pyramid: level l as
 * [2 * slots, rows_l, cols_l] u8, view-major (image v * slots + s is view v of slot s), for l = 0 .. SOSVO_LK_MAX_LEVELS - 1
 * whatever the settings (the workspace functions take no context); slots <= 32767 then.  The front end fills the levels the
 * context's settings use, in the rows of the range it computed (all rows unless GFT runs with the fused median); each level
 * equals sosvo_gray_pyramid of that frame's gray under the same range.  In a pair batch level 0 IS the front end's gray buffer.
 * sosvo_sequence_copy_slot[s] moves a slot's images with its record.  Raise `levels` only between sequences: a tracking call
 * reads the levels the settings name, a front end or copy has written those its settings named.
 * A pair's record depends only on its two slots' frames, its seed and the context's settings. */
#define SOSVO_FLAG_LK_F2F 0x80
#define SOSVO_LK_MAX_LEVELS 4
/* ---- cyclic panorama columns in the batch and sequence entry points --------------------------------
 *   SOSVO_FLAG_CYCLIC_F2F    a panorama is a full circle, column `cols` is column 0 again: the frame-to-frame |du| gate is the
 *                            cyclic one (sosvo_f2f_assemble_cyclic in place of sosvo_f2f_assemble); with SOSVO_FLAG_GATED_F2F
 *                            the gate is cyclic inside the matcher as well (sosvo_match_hamming_gated_cyclic, the view's period);
 *                            with SOSVO_FLAG_LK_F2F the tracked assemble is sosvo_f2f_assemble_tracked_cyclic, the store's
 *                            pyramids are those of sosvo_gray_pyramid_cyclic and the tracker runs with SOSVO_LK_CYCLIC_COLUMNS.
 * Honoured in sosvo_batch_cfg.ransac_flags (sosvo_frame_pair_batch*, sosvo_sequence_*); the bit is free in that word only: in
 * sosvo_rgbd_batch_cfg.flags bits 8 - 9 are the detector, and a pinhole image is not cyclic.  The period is pano_top[0] /
 * pano_bot[0] of the rig, positive integers.  With SOSVO_FLAG_LK_F2F it needs cols % 8 == 0 (every level the store may hold
 * is one period: 2^(SOSVO_LK_MAX_LEVELS - 1); the workspace functions take no context), and at call time 2 half + 3 columns
 * on the top level of the context's settings; together with SOSVO_FLAG_GATED_F2F | SOSVO_FLAG_RATIO_F2F it is refused (the
 * ratio form has no cyclic gate).  Otherwise SOSVO_ERR_ARG and a workspace size of 0.  The bit never reaches the RANSAC flags;
 * workspace sizes with the bit set equal those with it clear (no new buffers), and with the bit clear launches and results
 * are unchanged. */
#define SOSVO_FLAG_CYCLIC_F2F 0x200
/* ---- the seam-free front end: keypoints and stereo points up to the panorama seam ------------------
 * For a panorama P of `cols` columns (one period) and mask bits M, the seam-free front end is BY DEFINITION the plain front end
 * run on the padded inputs
 *   pad(P)[:, c']  = P[:, (c' - SOSVO_SEAM_HALO) mod cols]   for c' in [0, cols + 2 * SOSVO_SEAM_HALO)
 *   pad0(M)        = M in the columns [SOSVO_SEAM_HALO, SOSVO_SEAM_HALO + cols) and 0 in the halo
 * followed by the UNPAD of every keypoint's x, in float32: x = x' - 40, then + cols if x < 0, then - cols if x >= cols, and a
 * result equal to cols is written as 0.  Every original pixel is detected exactly once, and every pixel a stage reads for a
 * keypoint of the original columns is its true cyclic neighbour (the stages read at most about 35 columns around a keypoint;
 * the padded image's own border artefacts are its outer 5 to 8 columns).  The tuned image kernels are not edited: they run at
 * cols + 80 columns.  y, descriptors, counts and order are untouched; on the detector's grid (multiples of 1/32) the unpad is exact.
 * Limit: the greedy minimum distance and the per-mask maximum are not cyclic inside ONE mask that itself straddles the seam.
 *
 * The stages (each refuses NULL arguments and sizes out of range with SOSVO_ERR_ARG):
 *   sosvo_unwrap_prepare_seam_free  table [2, rows, cols + 80, 2] u32: byte for byte what sosvo_unwrap_prepare writes for maps
 *                                   padded by the rule above (an entry is a function of its map values alone); cols >= 40
 *   sosvo_mask_bits_seam_free       mask_bits [nsets, rows, cols] u32 -> out [nsets, rows, cols + 80]: pad0
 *   sosvo_keypoints_unpad           kp [nprob, cap, 2] f32, n [nprob] i32 (device): the unpad rule in place on the first
 *                                   min(n[p], cap) rows of every problem; the rows beyond are untouched.  period 1 .. 16384
 *   sosvo_gray_unpad                gray [nimg, rows, cols + 80] u8 -> out [nimg, rows, cols]: the interior columns; row_range as
 *                                   for sosvo_gauss7 (int32 [2][2] in DEVICE memory, view-major, nimg even; rows outside a view's
 *                                   range are not written), NULL = all rows
 *
 * In the batch and sequence entry points:
 *   SOSVO_FLAG_SEAM_FREE     sosvo_batch_cfg.ransac_flags (sosvo_frame_pair_batch*, sosvo_sequence_*).  cfg->cols stays the
 *                            period; the front end runs its image stages at cols + 80 internally and the caller passes the
 *                            table and mask bits made by the two helpers above.  Detection, description, sub-pixel refinement,
 *                            static-stereo matching, sort and sosvo_refine_stereo_lk keep padded coordinates (all of them are
 *                            shift-invariant or read the padded gray); top and bottom keypoints are unpadded as the last thing
 *                            before the stereo assemble.  A refined pair that ends up straddling the seam fails the plain stereo
 *                            gate and is dropped (the static-stereo gate is not cyclic).  With SOSVO_FLAG_LK_F2F level 0 of the
 *                            store is the interior crop, so a pair batch no longer uses the front end's buffer in place and its
 *                            workspace grows by one level 0.  The tracking step and everything behind it is unchanged.
 * The flag word is full except for its sign bit, so this IS the int32 sign bit; the next option needs a second word.  The
 * struct does not grow.  Refused with SOSVO_ERR_ARG and a workspace size of 0: the flag without SOSVO_FLAG_CYCLIC_F2F;
 * detector ORB (each pyramid level keeps a 31-pixel border of its own, which a 40-column halo covers on level 0 only);
 * edge > 31; cols < 40 or cols + 80 > 16384; everything SOSVO_FLAG_CYCLIC_F2F refuses; and, at call time (the workspace
 * functions take no context), SOSVO_FLAG_LK_STEREO settings with 2 + half + ceil(max_shift) > 35 (max_shift 0 = half).
 * sosvo_rgbd_batch_cfg.flags has no such bit.  With the flag clear launches, buffers and workspace sizes are unchanged. */
#define SOSVO_SEAM_HALO 40
#define SOSVO_FLAG_SEAM_FREE ((int32_t)(-2147483647 - 1))
int32_t sosvo_unwrap_prepare_seam_free(sosvo_ctx* ctx, const uint8_t* masks, const float* map_x, const float* map_y,
                                       int32_t H, int32_t W, int32_t rows, int32_t cols, uint32_t* table);
int32_t sosvo_mask_bits_seam_free(sosvo_ctx* ctx, const uint32_t* mask_bits, int32_t nsets, int32_t rows, int32_t cols,
                                  uint32_t* out);
int32_t sosvo_keypoints_unpad(sosvo_ctx* ctx, float* kp, const int32_t* n, int32_t nprob, int32_t cap, int32_t period);
int32_t sosvo_gray_unpad(sosvo_ctx* ctx, const uint8_t* gray, int32_t nimg, int32_t rows, int32_t cols,
                         const int32_t* row_range, uint8_t* out);
typedef struct sosvo_lk_options {
  int32_t half, levels, max_iter, reserved;
  double eps, min_eig, fb_max;
} sosvo_lk_options;
#define SOSVO_LK_OPTIONS_DEFAULT {10, 3, 30, 0, 0.01, 1e-4, 0.0}
int32_t sosvo_set_lk_options(sosvo_ctx* ctx, const sosvo_lk_options* options);

/* ---- sub-pixel static stereo: Lucas-Kanade disparity refinement (the cv2.calcOpticalFlowPyrLK(prevImg = top, nextImg = bottom)
 * call of match_features_panoramic_top_bottom, omnistereo/camera_models.py:3070, between the two views of ONE frame) ----------
 * sosvo_refine_stereo_lk runs after the static-stereo matching step (cross-check filter included: the keys are final) and
 * before sosvo_stereo_assemble.  It moves the BOTTOM keypoint of every matched pair to where the top keypoint's window is
 * found in the bottom image; the matcher's partner is the initial flow, so there is no pyramid.
 *   gray [nimg, rows, cols] u8, view-major: image f is the top view of frame f, image nimg / 2 + f its bottom view (nimg
 *   even, F = nimg / 2 frames); row_range as for sosvo_refine_subpix; kp_top, kp_bot [F * nmask, cap, 2] f32 and n_top, n_bot
 *   [F * nmask] i32; keys [F * nmask, cap] u32 in QUERY order (query = bottom, train = top, k = 1, SOSVO_KEY_NONE for a query
 *   without a match); status [F * nmask, cap] u8, optional.
 * Per problem p = frame * nmask + mask and bottom keypoint q < min(n_bot[p], cap), with t = keys[p, q] & SOSVO_KEY_IDX_MASK:
 *   1. keys[p, q] == SOSVO_KEY_NONE or t >= min(n_top[p], cap): kp_bot[p, q] is untouched, status 0.
 *   2. otherwise the point kp_top[p, t] of image frame is tracked into image nimg / 2 + frame by sosvo_track_lk's rule, word
 *      for word, with levels = 1, SOSVO_LK_INITIAL_FLOW and the guess g = kp_bot[p, q], no forward-backward check; half,
 *      max_iter, eps, min_eig from the settings.  Rounding, row ranges, the lost conditions are the tracker's (a non-finite
 *      coordinate: status 0).
 *   3. the result (x', y') is accepted iff the tracker's status is 1 and |x' - g.x| <= max_shift and |y' - g.y| <= max_shift
 *      (differences of the float32 values in double; a NaN fails).  Accepted: kp_bot[p, q] = (x', y'), status 1.  Otherwise
 *      kp_bot[p, q] keeps its bits, status 0 -- the revert of sosvo_refine_subpix rule 5, whose bound is the window half-size:
 *      max_shift = 0 means half.
 *   Rows at and beyond n_bot[p], kp_top, the descriptors and the counts are untouched.  Bottom queries are distinct: the order
 *   of work cannot matter.
 * The pre-gate: a pair that cannot pass sosvo_stereo_assemble's pixel gates after a move of at most max_shift per axis is not
 * tracked (untouched, status 0).  With du = u_top - u_bot, dv = v_top - v_bot, s = max_shift (all double) a pair is skipped iff
 *   stereo_max_hdiff > 0 and |du| > (stereo_max_hdiff + s) * (1 + 2^-40), or
 *   stereo_min_disp >= 0 and dv + s < stereo_min_disp - 2^-40 * (|dv| + s + stereo_min_disp);
 * each side is disabled exactly when the assemble stage's gate is.  The 2^-40 margins cover the rounding of the differences
 * (2^-53 relative): a pair that passes the gates after an accepted move is never skipped, and a skipped pair fails the gates
 * unrefined as well, so what sosvo_stereo_assemble writes does not depend on the pre-gate.
 *   options: NULL = the context's settings (sosvo_set_stereo_lk_options).  half 2 .. 10, max_iter 1 .. 30, eps and min_eig
 *   finite and >= 0, max_shift finite and >= 0 (0: half); nimg even, <= 65535; nmask >= 1; cap 1 .. 4096; F * nmask <= 65535;
 *   otherwise SOSVO_ERR_ARG.  Temporaries live in the context's scratch.
 *
 * In the batch and sequence entry points:
 *   SOSVO_FLAG_LK_STEREO     sosvo_batch_cfg.ransac_flags: the front end runs the stage between sosvo_sort_matches and the
 *                            stereo assemble, with the context's settings (SOSVO_STEREO_LK_OPTIONS_DEFAULT at creation:
 *                            half 4, max_iter 30, eps 0.01, min_eig 1e-4, max_shift = half).
 * Everything from the stereo gates on sees the refined bottom positions: bearings, triangulation, m_bot in the frame records,
 * the bottom view's frame-to-frame gates and SOSVO_FLAG_LK_F2F starts.  Descriptors stay those of the detector's positions.
 * It combines freely with every other option; with SOSVO_FLAG_SUBPIX that stage runs first and this one refines its result;
 * with the ORB detector it acts on kp_xy.  Bits 8 - 9 are free in the omni word only: sosvo_rgbd_batch_cfg.flags keeps its
 * detector there and has no stereo step.  The bit never reaches the RANSAC flags; the struct layouts and, with the bit
 * clear, workspace sizes, launches and results are unchanged.  With it set the workspace grows by the stage's status flags
 * ([window * nmask, kp_cap] u8).  sosvo_set_stereo_lk_options behaves like sosvo_set_lk_options: refused whole on a bad value
 * or a NULL pointer (SOSVO_ERR_ARG, the previous settings stay); sosvo_frame_pair_batch_streams* hands the settings to its
 * internal contexts at every call. */
#define SOSVO_FLAG_LK_STEREO 0x100
typedef struct sosvo_stereo_lk_options {
  int32_t half, max_iter;
  double eps, min_eig, max_shift;
} sosvo_stereo_lk_options;
#define SOSVO_STEREO_LK_OPTIONS_DEFAULT {4, 30, 0.01, 1e-4, 0.0}
int32_t sosvo_set_stereo_lk_options(sosvo_ctx* ctx, const sosvo_stereo_lk_options* options);
int32_t sosvo_refine_stereo_lk(sosvo_ctx* ctx, const uint8_t* gray, int32_t nimg, int32_t rows, int32_t cols,
                               const int32_t* row_range, int32_t nmask, int32_t cap, const float* kp_top, const int32_t* n_top,
                               float* kp_bot, const int32_t* n_bot, const uint32_t* keys, double stereo_min_disp,
                               double stereo_max_hdiff, const sosvo_stereo_lk_options* options, uint8_t* status);
#define SOSVO_SUBPIX_HALF_SHIFT 10
#define SOSVO_SUBPIX_HALF_MASK (3 << SOSVO_SUBPIX_HALF_SHIFT)
#define SOSVO_SUBPIX_HALF(h) (((h) - 2) << SOSVO_SUBPIX_HALF_SHIFT)
#define SOSVO_SUBPIX_HALF_OF(flags) ((((flags) & SOSVO_SUBPIX_HALF_MASK) >> SOSVO_SUBPIX_HALF_SHIFT) + 2)

/* ---- the whole hot path for a batch of frame pairs (the throughput entry point) ----------------
 * One call = for B independent pairs (frames 2i = reference / keyframe, 2i+1 = current):
 *   OmniStereoModel.set_current_omni_image + StereoPanoramicFrame.__init__ for both frames
 *   (omnistereo/camera_models.py:3107-3120, pose_est_tools.py:271-402: unwrap both mirrors, medianBlur, gray,
 *   goodFeaturesToTrack per azimuthal mask, ORB descriptors, per-bucket top/bottom matching, gates, bearings,
 *   midpoint triangulation, range filter), then TrackerStereoSE3.track_frame (pose_est_tools.py:736-847:
 *   frame-to-frame matching per view, |du| gate, stacking, non-central RANSAC, LM on the inliers).
 * It sequences the stage functions above on the context's stream; nothing is allocated and the host is never
 * synchronised.  Detector: cfg->detector (enum sosvo_detector; 0 = GFT, the reference default, pose_est_tools.py:684).
 * Each detector calls exactly the stages the Python ImageFrontEnd calls for it:
 *   GFT:          sosvo_detect_gft + sosvo_describe_orb_rows (angle cos_a / sin_a); with median_ksize 3 / 5 / 11 the
 *                 gray rows no consumer can reach are skipped (sosvo_gray_rows_needed)
 *   ORB:          sosvo_orb_mask_pyramid (rebuilt into the workspace on every call) + sosvo_detect_describe_orb
 *                 (nfeatures = max_corners, each keypoint's own angle; kp_cap <= 2048)
 *   FAST / AGAST: sosvo_detect_fast / sosvo_detect_agast (threshold 10) + sosvo_describe_orb (angle cos_a / sin_a)
 *   ORB, FAST and AGAST compute every gray row.  An unknown detector, or ORB with kp_cap > 2048, is SOSVO_ERR_ARG (and
 *   a workspace size of 0).
 *   omni         [2B, H, W, 3] u8 BGR (device)
 *   unwrap_table from sosvo_unwrap_prepare (model constant), mask_bits [2, rows, cols] u32 (set 0 = top mirror,
 *                set 1 = bottom mirror), pattern [512, 2] i8 (descriptor test points)
 *   workspace    caller-owned device memory, 256-byte aligned, >= sosvo_frame_pair_batch_workspace(cfg) bytes;
 *                contents on entry are irrelevant, intermediates (panoramas, keypoints, correspondences, ...) are
 *                left in it
 *   results      [B, 16] f64 (device): refined pose T = [R | t] row-major 3x4 (model units), n_inliers,
 *                n_correspondences, status (0 ok, 1 too few correspondences), best RANSAC iteration        */
typedef struct sosvo_batch_cfg {
  int32_t n_pairs;
  int32_t H, W;            /* omni frame: 1 <= H, W <= 16384, 3 * W * (H - 1) >= 8 (see sosvo_unwrap_prepare) */
  int32_t rows, cols;      /* panorama (both mirrors) */
  int32_t nmask;           /* azimuthal masks per mirror */
  int32_t kp_cap;          /* keypoint capacity per (frame, mirror, mask) */
  int32_t frame_cap;       /* stereo correspondences kept per frame (<= 16384) */
  int32_t median_ksize;    /* 11 (pose_est_tools.py:296) */
  int32_t max_corners;     /* per mask: FeatureMatcher.num_of_features (pose_est_tools.py:862) */
  int32_t edge;            /* ORB border, 31 */
  int32_t ransac_max_iter;
  int32_t ransac_adaptive; /* 1 = OpenGV's adaptive stop, 0 = exactly ransac_max_iter hypotheses */
  int32_t lm_max_iter;
  double quality;          /* 0.01 */
  double min_distance;     /* 5 */
  double ransac_threshold; /* 1 - cos(5 deg) (pose_est_tools.py:675-676) */
  uint64_t seed;           /* pair i samples with seed + i */
  float cos_a, sin_a;      /* descriptor orientation given to the GFT keypoints */
  int32_t ransac_flags;    /* SOSVO_FLAG_GP3P: generalised-P3P hypotheses (samples across both mirrors); 0: one-mirror P3P;
                              SOSVO_FLAG_CROSS_CHECK_STEREO / _F2F: mutual matches only (see above);
                              SOSVO_FLAG_GATED_STEREO / _F2F, SOSVO_GATED_MAX_DIST(d): search under the pixel gates (see above);
                              SOSVO_FLAG_RATIO_STEREO / _F2F, SOSVO_RATIO_64THS(r): the ratio rule (see above);
                              SOSVO_FLAG_SUBPIX, SOSVO_SUBPIX_HALF(h): sub-pixel keypoint refinement (see above);
                              SOSVO_FLAG_LK_F2F: Lucas-Kanade tracking in place of the frame-to-frame matcher (see above);
                              SOSVO_FLAG_LK_STEREO: sub-pixel static stereo, sosvo_refine_stereo_lk in the front end (see above) */
  int32_t detector;       /* enum sosvo_detector; 0 = GFT (this field was `reserved`, always 0, before) */
} sosvo_batch_cfg;

size_t sosvo_frame_pair_batch_workspace(const sosvo_batch_cfg* cfg);
int32_t sosvo_frame_pair_batch(sosvo_ctx* ctx, const sosvo_rig* rig_host, const sosvo_batch_cfg* cfg_host,
                               const uint8_t* omni, const uint32_t* unwrap_table, const uint32_t* mask_bits,
                               const int8_t* pattern, void* workspace, size_t workspace_bytes, double* results);

/* The same batch split over n_streams (1..4) INTERNAL HIP streams: the VALU-bound median of one part overlaps the
 * latency-bound stages of the others (the medians take turns), which is worth ~15 % over one stream at a few hundred
 * pairs.  Part s = pairs [lo_s, hi_s) (contiguous, sizes differ by at most one) samples with seed + pair index, so the
 * results are those of sosvo_frame_pair_batch, bit for bit.  The parts start after the work already queued on the context's
 * stream and the context's stream continues after all of them (events; no host synchronisation); the internal streams
 * and their scratch memory are created on first use and live as long as the context.
 * workspace: sosvo_frame_pair_batch_streams_workspace(cfg, n_streams) bytes, 256-aligned; n_pairs >= n_streams.  (H, W)
 * as for sosvo_frame_pair_batch: a frame size the table form refuses is refused before any part starts. */
size_t sosvo_frame_pair_batch_streams_workspace(const sosvo_batch_cfg* cfg, int32_t n_streams);
int32_t sosvo_frame_pair_batch_streams(sosvo_ctx* ctx, const sosvo_rig* rig_host, const sosvo_batch_cfg* cfg_host,
                                       int32_t n_streams, const uint8_t* omni, const uint32_t* unwrap_table,
                                       const uint32_t* mask_bits, const int8_t* pattern, void* workspace,
                                       size_t workspace_bytes, double* results);

/* Back-to-back batches without the join: ..._enqueue does everything sosvo_frame_pair_batch_streams does EXCEPT making the
 * context's stream wait for the parts, so the parts of the next call start while this call's later stages still run (part s
 * of call k + 1 follows part s of call k on the same internal stream; the medians' turn-taking goes on across calls) -- the
 * overlap the Python engine (pipeline.OverlappedFramePairs) has, for a host that calls the C ABI.  The caller then
 *   - hands every call inputs that are ready on the context's stream at the time of the call (as before),
 *   - alternates (at least) two `results` buffers if something still reads the previous call's records, and
 *   - calls ..._join(ctx) before reading records on the context's stream: it makes that stream wait for every part of
 *     the LATEST call (hence, in stream order, of all earlier ones), and
 *   - treats the INPUTS like the records: until the join nothing orders the context's stream after the parts, so `omni`
 *     (and the model tables) of an un-joined call must not be overwritten on the context's stream -- double-buffer the
 *     frames or join first.
 * The workspace may be the same for every call: part s of every call uses the same slice on the same internal stream.
 * That holds only for the same slice layout: part s's slice starts at workspace + the sizes of parts 0 .. s - 1, and a
 * part's size depends on the whole cfg (detector, kp_cap, nmask, frame_cap, rows / cols, H / W, median_ksize, its pairs).
 * So a call whose workspace pointer, n_streams or any part's size differ from the un-joined previous call's joins
 * internally first (correct, but without the overlap): changing the detector or a capacity between calls on one context
 * is safe, it only costs the overlap of that one call.  A call made while the context's stream is being captured into a
 * HIP graph fails with SOSVO_ERR_ARG while un-joined work is pending (join before capturing); after a join -- or after the
 * joined form sosvo_frame_pair_batch_streams -- every call is self-contained and capturable. */
int32_t sosvo_frame_pair_batch_streams_enqueue(sosvo_ctx* ctx, const sosvo_rig* rig_host, const sosvo_batch_cfg* cfg_host,
                                               int32_t n_streams, const uint8_t* omni, const uint32_t* unwrap_table,
                                               const uint32_t* mask_bits, const int8_t* pattern, void* workspace,
                                               size_t workspace_bytes, double* results);
int32_t sosvo_frame_pair_batch_streams_join(sosvo_ctx* ctx);

/* ---- Sequence mode: every frame's front end ONCE, tracking against keyframes -----------------------------
 * The reference's VO loop (run_VO, omnistereo/pose_est_tools.py:1416-1628) builds ONE StereoPanoramicFrame per image
 * (:1447-1463: unwrap, median, detection, static stereo, triangulation) and tracks it against the current KEYFRAME
 * (:1478, TrackerStereoSE3.track_frame :736-847); the keyframe policy (:1509-1565) depends on each tracked pose, so the
 * tracking is a serial chain while the front ends are independent.  These entry points split the batch path the same
 * way around a FRAME STORE in the caller's workspace: `slots` frame records (the frame's PanoramicCorrespondences as
 * SoA: pixels, descriptors, 3-D points, bearings, count), filled `window` frames at a time, tracked by slot numbers.
 *   cfg: sosvo_batch_cfg as for sosvo_frame_pair_batch; n_pairs = slot pairs one sosvo_sequence_track call may hold.
 *   workspace: sosvo_sequence_workspace(cfg, window, slots) bytes, 256-aligned, caller-owned; the SAME (cfg, window,
 *   slots) on every call.
 * sosvo_sequence_front_end: the front end of n_frames <= window omni frames [n_frames, H, W, 3] u8 (device) -> store
 *   slots first_slot .. first_slot + n_frames - 1.  Asynchronous.  (H, W): the frame size of the table form (see
 *   sosvo_unwrap_prepare); another is SOSVO_ERR_ARG, in the _slots form too.
 * sosvo_sequence_track: TrackerStereoSE3.track_frame for n_pairs (reference slot, current slot) pairs given as HOST
 *   arrays; pair i samples with seed + i -> results [n_pairs, 16] f64 (device) as sosvo_frame_pair_batch.  A pair's
 *   record depends only on its two slots' frames and its seed, so speculative tracking (every frame against its
 *   predecessor, in one call, before the keyframe decisions are known) gives exactly the records of the serial loop
 *   wherever the guess was right.  Asynchronous (up to 16 pairs travel as kernel arguments).
 * sosvo_sequence_copy_slot: store slot src -> dst (a frame promoted to keyframe outlives its window).  Asynchronous.
 * sosvo_sequence_frame_counts: the valid-correspondence counts (StereoPanoramicFrame.num_valid_keypoints, :372) of n
 *   slots -> HOST int32 array; SYNCHRONISES the context's stream (the one blocking call of the group).             */
size_t sosvo_sequence_workspace(const sosvo_batch_cfg* cfg, int32_t window, int32_t slots);
int32_t sosvo_sequence_front_end(sosvo_ctx* ctx, const sosvo_rig* rig_host, const sosvo_batch_cfg* cfg_host, int32_t window,
                                 int32_t slots, const uint8_t* omni, int32_t n_frames, int32_t first_slot,
                                 const uint32_t* unwrap_table, const uint32_t* mask_bits, const int8_t* pattern,
                                 void* workspace, size_t workspace_bytes);
int32_t sosvo_sequence_track(sosvo_ctx* ctx, const sosvo_rig* rig_host, const sosvo_batch_cfg* cfg_host, int32_t window,
                             int32_t slots, const int32_t* ref_slot_host, const int32_t* cur_slot_host, int32_t n_pairs,
                             uint64_t seed, void* workspace, size_t workspace_bytes, double* results);
int32_t sosvo_sequence_copy_slot(sosvo_ctx* ctx, const sosvo_batch_cfg* cfg_host, int32_t window, int32_t slots,
                                 int32_t src_slot, int32_t dst_slot, void* workspace, size_t workspace_bytes);
int32_t sosvo_sequence_frame_counts(sosvo_ctx* ctx, const sosvo_batch_cfg* cfg_host, int32_t window, int32_t slots,
                                    int32_t first_slot, int32_t n, void* workspace, size_t workspace_bytes,
                                    int32_t* counts_host);

/* ---- Several sequences through one frame store ("lanes") ---------------------------------------------------------
 * A frame record is a function of its image only and a tracking record of (reference record, current record, seed)
 * only, so S sequences that share ONE rig may share one store, one stream and one launch per stage: which call computes
 * a record never changes its bits.  A host that tracks S lanes with windows of W frames sizes the SAME workspace as
 * sosvo_sequence_workspace(cfg, S * W, S * (2 W + 1)) with cfg->n_pairs = S * W, gives lane s the slots
 * s (2 W + 1) .. s (2 W + 1) + 2 W (two window halves and its keyframe slot), and reads all lanes' counts with ONE
 * sosvo_sequence_frame_counts over the store.  The limits of the shape (window <= 16384, slots <= 65535,
 * n_pairs <= 8192) bound S * W.  What the single-sequence calls above cannot express:
 * sosvo_sequence_front_end_slots: sosvo_sequence_front_end with frame i's record written to slot slot_of_frame[i] (HOST
 *   array [n_frames]; every entry a slot of the store, none twice: SOSVO_ERR_ARG otherwise, nothing launched).  The
 *   frames of one call belong to different lanes, whose windows end at different times.  Asynchronous (the table
 *   travels as kernel arguments).
 * sosvo_sequence_track_seeds: sosvo_sequence_track with pair i sampling with seed_host[i] (HOST array [n_pairs]) instead
 *   of seed + i.  Asynchronous; up to 16 pairs travel with their seeds as kernel arguments, larger batches are copied.
 * sosvo_sequence_copy_slots: n_copies (source, destination) pairs (HOST arrays) in ONE launch; n_copies <=
 *   cfg->n_pairs.  A slot that is a destination twice, or both a source and a destination (src == dst included), is
 *   refused with SOSVO_ERR_ARG: the pairs are copied concurrently.  Asynchronous.                                    */
int32_t sosvo_sequence_front_end_slots(sosvo_ctx* ctx, const sosvo_rig* rig_host, const sosvo_batch_cfg* cfg_host,
                                       int32_t window, int32_t slots, const uint8_t* omni, int32_t n_frames,
                                       const int32_t* slot_of_frame_host, const uint32_t* unwrap_table,
                                       const uint32_t* mask_bits, const int8_t* pattern, void* workspace,
                                       size_t workspace_bytes);
int32_t sosvo_sequence_track_seeds(sosvo_ctx* ctx, const sosvo_rig* rig_host, const sosvo_batch_cfg* cfg_host, int32_t window,
                                   int32_t slots, const int32_t* ref_slot_host, const int32_t* cur_slot_host,
                                   const uint64_t* seed_host, int32_t n_pairs, void* workspace, size_t workspace_bytes,
                                   double* results);
int32_t sosvo_sequence_copy_slots(sosvo_ctx* ctx, const sosvo_batch_cfg* cfg_host, int32_t window, int32_t slots,
                                  const int32_t* src_slot_host, const int32_t* dst_slot_host, int32_t n_copies,
                                  void* workspace, size_t workspace_bytes);

/* ---- The RGB-D path for B independent frame pairs behind ONE call (BASELINE config 5) ------------------
 * RGBDFrame.establish_keypoints (omnistereo/pose_est_tools.py:600-623: [median,] gray, goodFeaturesToTrack on the
 * whole image or on RGBDFrame.mask, ORB descriptors, depth back-projection, NaN / range filter, bearings) for the
 * 2 B frames, then TrackerRGBDSE3.track_frame (:896-954: frame-to-frame matching, |du| gate, central RANSAC, LM)
 * for every pair (pair i tracks frame 2i+1 against frame 2i).  Sequences the stage entry points above on the
 * context's stream; same results as calling them one by one (vo_single_camera_sos_amd/pipeline.py:RGBDPairPipeline).
 *   bgr       [2B, rows, cols, 3] u8, depth [2B, rows, cols] f32 (camera depth units, 0 = no reading)
 *   mask_bits [1, rows, cols] u32 (bit 0 = pixel may hold a keypoint; all ones = RGBDFrame.mask None)
 *   pattern   [512, 2] i8 (the 256 ORB test pairs), workspace: sosvo_rgbd_pair_batch_workspace(cfg) bytes, 256-aligned
 *   results   [B, 16] f64 as sosvo_frame_pair_batch                                                             */
typedef struct sosvo_rgbd_batch_cfg {
  int32_t n_pairs;
  int32_t rows, cols;
  int32_t kp_cap;          /* keypoint capacity per frame; > 1024 selects the detector's whole-image variant */
  int32_t frame_cap;       /* keypoints with valid depth kept per frame */
  int32_t median_ksize;    /* 0: none (pose_est_tools.py:609 default) */
  int32_t max_corners;     /* FeatureMatcher.num_of_features, 1000 (pose_est_tools.py:691) */
  int32_t edge;            /* ORB border, 31 */
  int32_t ransac_max_iter;
  int32_t ransac_adaptive;
  int32_t lm_max_iter;
  int32_t flags;           /* SOSVO_FLAG_EPNP: "EPNP" (6-point samples); 0: "KNEIP" (P3P + 4th point); SOSVO_FLAG_GP3P: "GAO" / "GP3P";
                              SOSVO_FLAG_TWOPT: "TWOPT" -- passed through to sosvo_ransac_abs_pose;
                              bits 8-9: SOSVO_RGBD_DETECTOR(enum sosvo_detector), 0 = GFT (masked off before the solver).
                              SOSVO_FLAG_CROSS_CHECK_F2F: mutual matches only (masked off as well; ..._STEREO: SOSVO_ERR_ARG).
                              SOSVO_FLAG_GATED_F2F, SOSVO_GATED_MAX_DIST(d): search under the gate (likewise; ..._STEREO: SOSVO_ERR_ARG).
                              SOSVO_FLAG_RATIO_F2F, SOSVO_RATIO_64THS(r): the ratio rule (likewise; ..._STEREO: SOSVO_ERR_ARG).
                              SOSVO_FLAG_SUBPIX: SOSVO_ERR_ARG (depth is read at integer pixels).
                              SOSVO_FLAG_LK_F2F: SOSVO_ERR_ARG (the omni family's).
                              The detectors' stages are those of sosvo_frame_pair_batch on one whole-image mask (set 0
                              for every frame) */
  double quality, min_distance;        /* 0.01, 5 */
  double ransac_threshold;             /* 1 - cos(5 deg) */
  double pct_good_matches;             /* 1.0 (pose_est_tools.py:225) */
  double f2f_max_hdiff;                /* |du| gate in pixels: 0.5 * 2 * center_x (:956-958); <= 0: none */
  uint64_t seed;
  float cos_a, sin_a;
} sosvo_rgbd_batch_cfg;

size_t sosvo_rgbd_pair_batch_workspace(const sosvo_rgbd_batch_cfg* cfg);
int32_t sosvo_rgbd_pair_batch(sosvo_ctx* ctx, const sosvo_rgbd_cam* cam_host, const sosvo_rgbd_batch_cfg* cfg_host,
                              const uint8_t* bgr, const float* depth, const uint32_t* mask_bits, const int8_t* pattern,
                              void* workspace, size_t workspace_bytes, double* results);

/* ---- RGB-D sequence mode (the same split for the perspective path: demo_vo_rgbd.py's loop) ------------------
 * run_VO builds ONE RGBDFrame per image (pose_est_tools.py:1440-1446, :600-623) and tracks it against the current keyframe
 * (TrackerRGBDSE3.track_frame, :896-954).  Frame store, window, slots, seeds and the speculation argument exactly as in the
 * omnistereo sequence mode above; cfg: sosvo_rgbd_batch_cfg as for sosvo_rgbd_pair_batch (n_pairs = slot pairs one
 * ..._track call may hold).
 *   bgr [n_frames, rows, cols, 3] u8, depth [n_frames, rows, cols] f32 (device)                                      */
size_t sosvo_rgbd_sequence_workspace(const sosvo_rgbd_batch_cfg* cfg, int32_t window, int32_t slots);
int32_t sosvo_rgbd_sequence_front_end(sosvo_ctx* ctx, const sosvo_rgbd_cam* cam_host, const sosvo_rgbd_batch_cfg* cfg_host,
                                      int32_t window, int32_t slots, const uint8_t* bgr, const float* depth, int32_t n_frames,
                                      int32_t first_slot, const uint32_t* mask_bits, const int8_t* pattern, void* workspace,
                                      size_t workspace_bytes);
int32_t sosvo_rgbd_sequence_track(sosvo_ctx* ctx, const sosvo_rgbd_batch_cfg* cfg_host, int32_t window, int32_t slots,
                                  const int32_t* ref_slot_host, const int32_t* cur_slot_host, int32_t n_pairs, uint64_t seed,
                                  void* workspace, size_t workspace_bytes, double* results);
int32_t sosvo_rgbd_sequence_copy_slot(sosvo_ctx* ctx, const sosvo_rgbd_batch_cfg* cfg_host, int32_t window, int32_t slots,
                                      int32_t src_slot, int32_t dst_slot, void* workspace, size_t workspace_bytes);
int32_t sosvo_rgbd_sequence_frame_counts(sosvo_ctx* ctx, const sosvo_rgbd_batch_cfg* cfg_host, int32_t window, int32_t slots,
                                         int32_t first_slot, int32_t n, void* workspace, size_t workspace_bytes,
                                         int32_t* counts_host);
/* Several RGB-D sequences of one camera through one store: as "Several sequences through one frame store" above, on
 * sosvo_rgbd_sequence_workspace(cfg, S * W, S * (2 W + 1)) with cfg->n_pairs = S * W.                              */
int32_t sosvo_rgbd_sequence_front_end_slots(sosvo_ctx* ctx, const sosvo_rgbd_cam* cam_host,
                                            const sosvo_rgbd_batch_cfg* cfg_host, int32_t window, int32_t slots,
                                            const uint8_t* bgr, const float* depth, int32_t n_frames,
                                            const int32_t* slot_of_frame_host, const uint32_t* mask_bits,
                                            const int8_t* pattern, void* workspace, size_t workspace_bytes);
int32_t sosvo_rgbd_sequence_track_seeds(sosvo_ctx* ctx, const sosvo_rgbd_batch_cfg* cfg_host, int32_t window, int32_t slots,
                                        const int32_t* ref_slot_host, const int32_t* cur_slot_host,
                                        const uint64_t* seed_host, int32_t n_pairs, void* workspace,
                                        size_t workspace_bytes, double* results);
int32_t sosvo_rgbd_sequence_copy_slots(sosvo_ctx* ctx, const sosvo_rgbd_batch_cfg* cfg_host, int32_t window, int32_t slots,
                                       const int32_t* src_slot_host, const int32_t* dst_slot_host, int32_t n_copies,
                                       void* workspace, size_t workspace_bytes);

/* ---- dense omnistereo: SGM disparity map and point cloud -----------------------------------------
 * Restates OmniStereoModel.get_depth_map_from_panoramas (camera_models.py:3395) with the SGBM settings of
 * common_cv.StereoMatchTuner (common_cv.py:482-497: num_of_disparities 64, uniqueness 15, disp12MaxDiff; :644 the match of
 * the rotated panoramas), resolve_pano_correspondences_from_disparity_map (:2492) and triangulate_from_depth_map (:2567).
 * The reference runs cv2.StereoSGBM inside a tuner window; the algorithm here is THIS header's definition, modelled on
 * SGBM, and the device reproduces tests/refdense.py (the same text in numpy) bit for bit.  It is no claim of parity with cv2.
 *
 * The rig is coaxial and its panoramas are rectified cylinders: epipolar lines are columns, and the top pixel (r, c) with
 * disparity d corresponds to the bottom pixel (r - d, c) (the reference's m_bot = (u, v_top - disp); the sign of
 * sosvo_rig.stereo_min_disp).  D = 64 disparities d = d0 + k, k = 0 .. 63, d0 = min_disparity.
 *
 * sosvo_census_9x7: gray [nimg, rows, cols] u8 -> census_out [nimg, rows, cols] u64.
 *   a. A 9-row by 7-column window, 62 bits: taps in the order dy = -4 .. 4 outer, dx = -3 .. 3 inner, centre skipped, each
 *      appending census = census << 1 | (g[r + dy, c + dx] < g[r, c]); the first tap ends in bit 61.  Rows clamp (replicated
 *      border).  Columns clamp, or with SOSVO_DENSE_CYCLIC_COLUMNS in flags wrap modulo cols (the seam is no border: the
 *      meaning of SOSVO_LK_CYCLIC_COLUMNS).  The flag changes nothing but these taps.
 *
 * sosvo_dense_stereo: top, bot [n, rows, cols] u8 gray panoramas (sosvo_unwrap_median_gray's output: top = its first n
 *   images, bot = the next n; any two buffers will do), mask [rows, cols] u8 shared by the n frames or NULL (all valid).
 *   b. C(r, c, k) = popcount(census_top(r, c) ^ census_bot(r - d, c)); 64 where r - d < 0.
 *   c. Four paths (down, up, left to right, right to left).  Each starts at the image border with L = C; after that, with
 *      m = min_j L_prev(j):  L(p, k) = C(p, k) + min(L_prev(k), L_prev(k - 1) + P1, L_prev(k + 1) + P1, m + P2) - m,
 *      a missing neighbour (k - 1 < 0, k + 1 > 63) taking no part.  S = the sum of the four L (<= 4 * (64 + P2) <= 33020).
 *      P1 = P2 = 0 (what the reference's tuner passes) switches the smoothness off and is accepted.
 *   d. k* = the smallest k with the minimal S, mS = S(k*).
 *   e. The pixel is dropped if some k with |k - k*| > 1 has S(k) * (100 - uniqueness) < mS * 100 (int32), or
 *      r - (d0 + k*) < 0, or the mask is 0 at (r, c).
 *   f. Left-right check, lr_max >= 0 (negative: none, the reference's disp12MaxDiff = -1): per column, over the pixels that
 *      survived e in ascending r, the bottom row rb = r - (d0 + k*) keeps the k* of the surviving pixel with the smallest
 *      mS (ties: the smaller r); a pixel is dropped if |kept(rb) - k*| > lr_max.
 *   g. Sub-pixel, 1/16 row: for 1 <= k* <= 62, a = S(k* - 1), b = S(k* + 1), den = max(a + b - 2 mS, 1),
 *      off = floor(((a - b) * 16 + den) / (2 den)) in [-8, 8]; off = 0 at k* = 0 and 63.
 *   d16_out [n, rows, cols] i16 = (d0 + k*) * 16 + off, -1 for a dropped pixel.  S_out [n, rows, cols, 64] u16 or NULL: the
 *   aggregated volume of step c (so that a failing parity test says which stage differs).  No pre-filter; the speckle
 *   filter is a call of its own, sosvo_dense_speckle below.
 *   Temporaries (census words, the cost volume, S without S_out, the left-right keys: about 210 bytes per pixel) live in the
 *   context's scratch.
 *
 * sosvo_dense_stereo_paths: sosvo_dense_stereo with the number of aggregation paths as an argument.
 *   paths = 4: exactly sosvo_dense_stereo, the same launches and the same bytes.  paths = 8: the reference tuner's "Full DP"
 *   switch (common_cv.StereoMatchTuner.full_dyn_prog, cv2.STEREO_SGBM_MODE_HH); a caller maps it as
 *   paths = full_dyn_prog ? 8 : 4.  Steps a, b, d, e, f and g are unchanged; step c gains four diagonal paths, with
 *   (dr, dc) in {(+1, +1), (+1, -1), (-1, +1), (-1, -1)}:
 *   c8. The predecessor of pixel (r, c) on path (dr, dc) is (r - dr, c - dc).  The path starts at (r, c), L = C, where
 *      r - dr lies outside [0, rows); without SOSVO_DENSE_CYCLIC_COLUMNS also where c - dc lies outside [0, cols).  With
 *      the flag the predecessor's column is (c - dc) mod cols: the seam is no border, as for the census taps, and for
 *      cols = 1 the predecessor is the pixel above or below in the same column.  Elsewhere the recurrence of step c runs on
 *      the predecessor's L.  S = the sum of the eight L (<= 8 * (64 + P2)) and stays u16, so that eight paths require
 *      P2 <= SOSVO_DENSE_MAX_P2_EIGHT_PATHS = 8127 (S <= 65528); four paths keep 8191.
 *      The same thing as lines (tests/refdense8.py, the kernel): line j in [0, cols) at step i in [0, rows) visits row i
 *      (dr = +1) or rows - 1 - i (dr = -1) and column (j + dc * i) mod cols; in the clamped form it starts again with L = C
 *      at every step i > 0 whose column is 0 (dc = +1) or cols - 1 (dc = -1).  Every pixel is visited by exactly one line
 *      of a pass, exactly once, whether rows > cols or not.
 *   Refusals (SOSVO_ERR_ARG before any launch): those of sosvo_dense_stereo, paths not 4 or 8, paths = 8 with P2 > 8127.
 *   The scratch is that of sosvo_dense_stereo.
 *
 * sosvo_dense_triangulate: d16 [n, rows, cols] i16 -> X_out [n, rows, cols, 3] f64 in the rig's frame [C].  rig_host: the
 *   sosvo_rig of sosvo_stereo_assemble (pano_top, pano_bot, F_top, F_bot, min_range, max_range are read).  For d16 >= 0,
 *   d16 >= min_d16 and (max_d16 <= 0 or d16 <= max_d16): top pixel (c, r), bottom pixel (c, r - d16 / 16.0) in double; angles,
 *   midpoint and range filter exactly as sosvo_pano_to_bearing -> sosvo_triangulate_midpoint -> sosvo_range_filter give them
 *   (the same device functions, the same bits).  Everything else is NaN in all three components; a bottom row outside
 *   [0, rows) is NaN because the angle is.
 *
 * SOSVO_ERR_ARG before any launch: rows or cols outside 1 .. 16384; n (nimg) < 1 (or > 32767; nimg > 65535); P1 < 0,
 * P1 > P2, P2 > 8191; uniqueness outside [0, 100); min_disparity outside [0, 1024]; unknown flag bits; a NULL required
 * pointer; a rig whose two panoramas differ in geometry.  Asynchronous on the context's stream.                       */
#define SOSVO_DENSE_CYCLIC_COLUMNS 1
#define SOSVO_DENSE_DISPARITIES 64
int32_t sosvo_census_9x7(sosvo_ctx* ctx, const uint8_t* gray, int32_t nimg, int32_t rows, int32_t cols, int32_t flags,
                         uint64_t* census_out);
int32_t sosvo_dense_stereo(sosvo_ctx* ctx, const uint8_t* top, const uint8_t* bot, int32_t n, int32_t rows, int32_t cols,
                           const uint8_t* mask, int32_t min_disparity, int32_t P1, int32_t P2, int32_t uniqueness,
                           int32_t lr_max, int32_t flags, int16_t* d16_out, uint16_t* S_out);
#define SOSVO_DENSE_MAX_P2_EIGHT_PATHS 8127
int32_t sosvo_dense_stereo_paths(sosvo_ctx* ctx, const uint8_t* top, const uint8_t* bot, int32_t n, int32_t rows, int32_t cols,
                                 const uint8_t* mask, int32_t min_disparity, int32_t P1, int32_t P2, int32_t uniqueness,
                                 int32_t lr_max, int32_t flags, int32_t paths, int16_t* d16_out, uint16_t* S_out);
int32_t sosvo_dense_triangulate(sosvo_ctx* ctx, const sosvo_rig* rig_host, const int16_t* d16, int32_t n, int32_t rows,
                                int32_t cols, int32_t min_d16, int32_t max_d16, double* X_out);

/* ---- dense omnistereo: speckle filter -------------------------------------------------------------
 * The reference's tuner sliders "Speckle Window Size" / "Speckle Range" (common_cv.StereoMatchTuner, common_cv.py:496-497,
 * passed to cv2.StereoSGBM as speckleWindowSize / speckleRange): what cv2.filterSpeckles' flood fill computes, stated here
 * and in tests/refspeckle.py (the same text in numpy), which the device reproduces bit for bit.
 *
 * sosvo_dense_speckle: d16 [n, rows, cols] i16 (sosvo_dense_stereo's map; any map will do) -> d16_out [n, rows, cols] i16.
 * Per frame; no frame sees another.
 *   a. A pixel is valid iff d16 >= 0 (ANY negative value is invalid, not only -1).
 *   b. Two 4-neighbours are joined iff both are valid and |d16_a - d16_b| <= max_diff, the difference taken in int32.  The
 *      pairs are (r, c)-(r + 1, c) and (r, c)-(r, c + 1); with SOSVO_DENSE_CYCLIC_COLUMNS in flags also (r, cols - 1)-(r, 0)
 *      when cols > 1 (the panorama's seam is no border).
 *   c. Components are the connected components of that graph.  The relation is not transitive, the graph is: a ramp
 *      0, 16, 32, 48 with max_diff 16 is one component.
 *   d. A valid pixel whose component has size <= max_size becomes -1.  Everything else, the original values of invalid
 *      pixels included, is copied unchanged.  max_size = 0 therefore drops nothing; it is accepted and still runs.
 *   labels_out [n, rows, cols] u32 or NULL: the smallest row-major index r * cols + c of the pixel's component, 0xFFFFFFFF
 *   for an invalid pixel (so that a failing parity test says whether the labelling or the threshold differs).
 *   d16_out == d16 is allowed: the call then filters in place.  Temporaries (a u32 label and a u32 size per pixel, 8 bytes
 *   per pixel) live in the context's scratch.  The result is a pure function of the input: the label is a minimum, so it
 *   depends on no order of execution.
 *
 * SOSVO_ERR_ARG before any launch: rows or cols outside 1 .. 16384; n < 1 or > 32767; max_size < 0; max_diff outside
 * 0 .. 32767; unknown flag bits; d16 or d16_out NULL.  Asynchronous on the context's stream.                           */
int32_t sosvo_dense_speckle(sosvo_ctx* ctx, const int16_t* d16, int32_t n, int32_t rows, int32_t cols, int32_t max_size,
                            int32_t max_diff, int32_t flags, int16_t* d16_out, uint32_t* labels_out);

#ifdef __cplusplus
}
#endif
#endif /* SOSVO_H */
