// sosvo_dense_stereo's scratch (dense.hip), host-compilable like scratch_carver.h so that
// tests/test_scratch_carver.py can check it against the sizes include/sosvo.h documents.
#ifndef SOSVO_DENSE_SCRATCH_H
#define SOSVO_DENSE_SCRATCH_H

#include <stdint.h>

#include "scratch_carver.h"

struct sosvo_dense_scratch {
  uint64_t *census_top, *census_bot;  // [total] census words of the two views
  uint8_t* C;                         // [total, disparities] the cost volume
  uint16_t* S;                        // [total, disparities] the aggregated volume; not carved when the caller gives S_out
  uint8_t* kstar;                     // [total] k* per pixel
  uint32_t* best;                     // [total] the left-right keys; not carved without the left-right check
};

// total = n * rows * cols pixels
static inline sosvo_dense_scratch sosvo_dense_carve(Carver& cv, size_t total, size_t disparities, bool s_given, bool want_lr) {
  sosvo_dense_scratch b;
  b.census_top = cv.take<uint64_t>(total);
  b.census_bot = cv.take<uint64_t>(total);
  b.C = cv.take<uint8_t>(total * disparities);
  b.S = cv.take<uint16_t>(s_given ? 0 : total * disparities);
  b.kstar = cv.take<uint8_t>(total);
  b.best = cv.take<uint32_t>(want_lr ? total : 0);
  return b;
}

#endif
