/* CAST's per-element conversion and parameter check, shared by the device
 * kernel (cast_kernel, glue.hip) and the host twin (CpuCast), so the two
 * workers convert alike by construction.
 *   float32 -> integer truncates toward zero; NaN gives 0; a value outside the
 * target's range saturates at the nearer end (what the device's conversion
 * instructions do for 32 bits; stated here for every width, so that the host
 * never executes an undefined conversion).  This is this backend's rule:
 * TFLite's cast.cc is a static_cast, undefined outside the range.
 *   integer -> integer is the C++ conversion (a narrowing keeps the low bits);
 * integer -> float32 rounds to nearest. */
#pragma once

#include <stdint.h>

#include "band_hip_kernels.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BH_CAST_FN __host__ __device__ inline
#else
#define BH_CAST_FN inline
#endif

template <class D>
BH_CAST_FN D bh_cast_from_f32(float f);
template <>
BH_CAST_FN float bh_cast_from_f32<float>(float f) {
  return f;
}
template <>
BH_CAST_FN uint8_t bh_cast_from_f32<uint8_t>(float f) {
  if (!(f > -1.0f)) return 0; /* NaN too */
  if (f >= 256.0f) return 255;
  return (uint8_t)(int32_t)f;
}
template <>
BH_CAST_FN int32_t bh_cast_from_f32<int32_t>(float f) {
  if (f != f) return 0;
  if (f >= 2147483648.0f) return INT32_MAX;
  if (f < -2147483648.0f) return INT32_MIN;
  return (int32_t)f; /* |f| < 2^31, or f == -2^31 */
}
template <>
BH_CAST_FN int64_t bh_cast_from_f32<int64_t>(float f) {
  if (f != f) return 0;
  if (f >= 9223372036854775808.0f) return INT64_MAX;
  if (f < -9223372036854775808.0f) return INT64_MIN;
  return (int64_t)f;
}

/* one element of type S as a D */
template <class S, class D>
BH_CAST_FN D bh_cast_one(S v) {
  return (D)v;
}
template <>
BH_CAST_FN uint8_t bh_cast_one<float, uint8_t>(float v) {
  return bh_cast_from_f32<uint8_t>(v);
}
template <>
BH_CAST_FN int32_t bh_cast_one<float, int32_t>(float v) {
  return bh_cast_from_f32<int32_t>(v);
}
template <>
BH_CAST_FN int64_t bh_cast_one<float, int64_t>(float v) {
  return bh_cast_from_f32<int64_t>(v);
}
/* (narrowing keeps the low bits, through the unsigned type: no implementation-defined step) */
template <>
BH_CAST_FN int32_t bh_cast_one<int64_t, int32_t>(int64_t v) {
  return (int32_t)(uint32_t)(uint64_t)v;
}

inline int bh_cast_type_bytes(int type) {
  return type == BH_CAST_U8 ? 1 : (type == BH_CAST_I32 || type == BH_CAST_F32) ? 4 : type == BH_CAST_I64 ? 8 : 0;
}

/* NULL = runnable, else the reason */
inline const char* bh_cast_why(const bh_cast_params* p) {
  if (!p) return "null parameter block";
  if (!p->input || !p->output) return "null pointer";
  if (p->count < 0) return "negative count";
  if (!bh_cast_type_bytes(p->in_type) || !bh_cast_type_bytes(p->out_type))
    return "types must be BH_CAST_U8, _I32, _I64 or _F32";
  if (((uintptr_t)p->input % (uintptr_t)(bh_cast_type_bytes(p->in_type) == 1 ? 1 : 4)) ||
      ((uintptr_t)p->output % (uintptr_t)(bh_cast_type_bytes(p->out_type) == 1 ? 1 : 4)))
    return "a pointer is not aligned to its element (4 bytes for the 4- and 8-byte types)";
  return 0;
}
