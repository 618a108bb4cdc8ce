/* Prelude of the solver headers that the device and the CPU oracle BOTH compile (trig_core.h, ransac_core.h,
 * epnp_core.h, gp3p_core.h, relpose_core.h): the function qualifiers are the only words the two sides spell differently.
 * hipcc sees device functions, gcc (-std=c11, oracle/Makefile) plain static inline ones.  ransac_core.h uses
 * SV_FN_INLINE throughout and the other four SV_FN: the scoring kernels were tuned with every helper of ransac_core.h
 * inlined, and the difference decides the generated code -- keep it. */
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SV_FN __device__ static
#define SV_FN_INLINE __device__ __forceinline__ static
#else
#define SV_FN static inline
#define SV_FN_INLINE static inline
#endif
