// Column layout of the four-columns-per-lane blur (gauss7_wide_kernel, detect.hip), as plain integer arithmetic that the
// host compiles too: tests/test_rolling_layout.py checks every (cols, strip, lane) on the CPU.
//
// A wave covers kBlurWideSpan = 256 consecutive "virtual" columns of a row, lane l the four columns x0 .. x0 + 3 with
// x0 = strip * kBlurWideStripW - 3 + 4 l, and owns the kBlurWideStripW = 250 outputs strip * 250 .. strip * 250 + 249
// (byte 3 of lane 0 .. byte 0 of lane 63).  A virtual column outside the image stands for its reflect-101 mirror image.
// Every lane loads ONE dword, at column `off` of the row, always inside the row (0 <= off <= cols - 4), and `sel` is the
// v_perm_b32 selector (byte k of the result = byte sel[k] of the loaded dword) that turns it into the lane's four virtual
// columns.  The mirror image of the columns -3 .. -1 lies in the columns 1 .. 3 and that of cols .. cols + 2 in
// cols - 4 .. cols - 2, so with cols >= 4 a single reflection reaches every column an output can need (x - 3 .. x + 3 of
// 0 <= x < cols) and all four of a lane's columns lie within the four bytes at the clamped offset; columns further out
// feed no output and get some byte of the load.  The launcher asks for cols >= kBlurWideMinCols = 8 (a row then holds
// two dwords: the left and the right border never meet in one lane's load) and runs the one-column form below that.
// In a strip whose 256 columns all lie inside the image off = x0 and sel is the identity: that instantiation skips the
// permute.
#ifndef SOSVO_ROLLING_LAYOUT_H
#define SOSVO_ROLLING_LAYOUT_H

#include <stdint.h>

#ifdef __HIPCC__
#define SOSVO_LAYOUT_FN __host__ __device__ static inline
#else
#define SOSVO_LAYOUT_FN static inline
#endif

#define SOSVO_BLUR_WIDE_SPAN 256
#define SOSVO_BLUR_WIDE_STRIP_W 250
#define SOSVO_BLUR_WIDE_MIN_COLS 8

typedef struct sosvo_blur_wide_lane {
  int32_t off;   /* column of the lane's dword load, 0 .. cols - 4 */
  uint32_t sel;  /* v_perm_b32 selector: loaded dword -> the virtual columns x0 .. x0 + 3 */
  uint32_t own;  /* bit j: virtual column x0 + j is an output of this wave inside the image */
} sosvo_blur_wide_lane;

SOSVO_LAYOUT_FN sosvo_blur_wide_lane sosvo_blur_wide_layout(int cols, int strip, int lane) {
  sosvo_blur_wide_lane r;
  const int first = strip * SOSVO_BLUR_WIDE_STRIP_W;
  const int x0 = first - 3 + 4 * lane;
  int off = x0;
  if (off > cols - 4) off = cols - 4;
  if (off < 0) off = 0;
  r.off = off;
  r.sel = 0u;
  r.own = 0u;
  for (int j = 0; j < 4; ++j) {
    const int c = x0 + j;
    int m = c < 0 ? -c : (c >= cols ? 2 * (cols - 1) - c : c);  /* reflect-101, once */
    int b = m - off;
    if (b < 0) b = 0;
    if (b > 3) b = 3;
    r.sel |= (uint32_t)b << (8 * j);
    if (c >= first && c < first + SOSVO_BLUR_WIDE_STRIP_W && c < cols) r.own |= 1u << j;
  }
  return r;
}

/* strips of a row, and whether a strip needs the permute (some lane's four columns are not all inside the image) */
SOSVO_LAYOUT_FN int sosvo_blur_wide_strips(int cols) { return (cols + SOSVO_BLUR_WIDE_STRIP_W - 1) / SOSVO_BLUR_WIDE_STRIP_W; }
SOSVO_LAYOUT_FN int sosvo_blur_wide_edge_strip(int cols, int strip) {
  const int xb = strip * SOSVO_BLUR_WIDE_STRIP_W - 3;
  return xb < 0 || xb + SOSVO_BLUR_WIDE_SPAN > cols;
}

#endif
