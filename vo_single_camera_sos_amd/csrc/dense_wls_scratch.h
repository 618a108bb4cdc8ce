// sosvo_dense_wls's scratch (dense_wls.hip), host-compilable like dense_scratch.h: 40 bytes per pixel
// and the 2 KiB table; the cyclic form's third right-hand side adds 8 bytes per pixel and 16 per row (at most 56 per pixel
// together, at its narrowest map of 3 columns).
#ifndef SOSVO_DENSE_WLS_SCRATCH_H
#define SOSVO_DENSE_WLS_SCRATCH_H

#include <stdint.h>

#include "scratch_carver.h"

struct sosvo_dense_wls_scratch {
  double* weights;    // [256] the caller's table
  double *N, *D;      // [total] the two right-hand sides, replaced by every solve
  double* cp;         // [total] c' of the forward sweep
  double *fN, *fD;    // [total] f' of the two right-hand sides
  double* fz;         // [total] f', then z, of the cyclic form's third right-hand side; not carved without it
  double* ratio;      // [lines, 2] vy / vz of the two right-hand sides per row; not carved without the cyclic form
};

// total = n * rows * cols pixels, lines = n * rows
static inline sosvo_dense_wls_scratch sosvo_dense_wls_carve(Carver& cv, size_t total, size_t lines, bool cyclic_rows) {
  sosvo_dense_wls_scratch b;
  b.weights = cv.take<double>(256);
  b.N = cv.take<double>(total);
  b.D = cv.take<double>(total);
  b.cp = cv.take<double>(total);
  b.fN = cv.take<double>(total);
  b.fD = cv.take<double>(total);
  b.fz = cv.take<double>(cyclic_rows ? total : 0);
  b.ratio = cv.take<double>(cyclic_rows ? 2 * lines : 0);
  return b;
}

#endif
