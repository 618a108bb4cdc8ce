// sosvo_dense_stereo_wide's scratch (dense_wide.hip), host-compilable like dense_scratch.h so that
// tests/test_dense_wide_reference.py can check it against the sizes include/sosvo_dense_wide.h documents.  It is
// dense_scratch.h's layout with k* widened to 16 bits: 255 is a winner at 256 disparities, so 0xFFFF marks a dropped pixel.
#ifndef SOSVO_DENSE_WIDE_SCRATCH_H
#define SOSVO_DENSE_WIDE_SCRATCH_H

#include <stdint.h>

#include "scratch_carver.h"

struct sosvo_dense_wide_scratch {
  uint64_t *census_top, *census_bot;  // [total] census words of the two views
  uint8_t* C;                         // [total, disparities] the cost volume
  uint16_t* S;                        // [total, disparities] the aggregated volume; not carved when the caller gives S_out
  uint16_t* kstar;                    // [total] k* per pixel, 0xFFFF = dropped
  uint32_t* best;                     // [total] the left-right keys; not carved without the left-right check
};

// total = n * rows * cols pixels
static inline sosvo_dense_wide_scratch sosvo_dense_wide_carve(Carver& cv, size_t total, size_t disparities, bool s_given, bool want_lr) {
  sosvo_dense_wide_scratch b;
  b.census_top = cv.take<uint64_t>(total);
  b.census_bot = cv.take<uint64_t>(total);
  b.C = cv.take<uint8_t>(total * disparities);
  b.S = cv.take<uint16_t>(s_given ? 0 : total * disparities);
  b.kstar = cv.take<uint16_t>(total);
  b.best = cv.take<uint32_t>(want_lr ? total : 0);
  return b;
}

#endif
