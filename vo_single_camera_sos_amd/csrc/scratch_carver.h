// How every stage lays its buffers out in a scratch allocation (the context's own, or the caller's workspace in
// pipeline.hip), as plain C++ that a host compiler builds too: tests/test_scratch_carver.py checks it on the CPU.
//
// A layout is a function that takes its buffers from a Carver in a fixed order, each stated once with its element type and
// count.  Run over a null base it MEASURES: every pointer comes back null and `off` ends at the bytes to reserve.  Run over
// the allocation it PLACES: the same calls give the typed pointers.  A buffer starts on a multiple of 256 bytes from the
// base, and a buffer of no elements takes no room.
#ifndef SOSVO_SCRATCH_CARVER_H
#define SOSVO_SCRATCH_CARVER_H

#include <stddef.h>

static inline size_t sosvo_round256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

struct Carver {
  char* base;
  size_t off = 0;
  template <typename T>
  T* take(size_t count) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += sosvo_round256(count * sizeof(T));
    return p;
  }
};

#endif
