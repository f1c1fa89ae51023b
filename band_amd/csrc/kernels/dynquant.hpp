// The run-time quantisation rule of the dynamic-range ("hybrid") ops, shared
// by dynquant_rows_kernel (fc_hybrid.hip: a row per wave) and the per-item
// kernels of conv_hybrid.hip: the wave reductions, the derivation of
// (scale, 1 / scale, offset) from a row's or item's (min, max), and the
// quantisation of one value.  band_hip_kernels.h holds the rule; the files
// that include this are built with -ffp-contract=off and the correctly
// rounded division.
#pragma once

#include "common.hpp"

namespace bh {

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// (s, inv, off) of mn = min(0, min x), mx = max(0, max x).  inv 0: every q is
// the offset, 0.  The asymmetric form is float64 past the float32 difference.
__device__ __forceinline__ void dq_derive(float mn, float mx, bool asymmetric, float& s, float& inv, int32_t& off) {
  s = 1.f;
  inv = 0.f;
  off = 0;
  if (!asymmetric) {
    const float r = fmaxf(-mn, mx);
    if (r != 0.f) {
      s = r / 127.f;
      inv = 127.f / r;
    }
  } else if (mn != mx) {
    const float range = mx - mn;
    const double scale = (double)range / 255.0;
    const double a = (double)mn / scale, b = (double)mx / scale;
    const double z_min = -128.0 - a, z_max = 127.0 - b;
    const double e_min = 128.0 + fabs(a), e_max = 127.0 + fabs(b);
    const double z = e_min < e_max ? z_min : z_max;
    off = z <= -128.0 ? -128 : (z >= 127.0 ? 127 : (int32_t)(int8_t)round(z));
    s = (float)scale;
    inv = 1.0f / s;
  }
}

// one value by the row's (inv, offset): round half away from zero, then the clamp
__device__ __forceinline__ int32_t dq_one(float x, float inv, float off, int32_t lo) {
  const float t = x * inv;
  const int32_t v = (int32_t)roundf(off + t);
  return v < lo ? lo : (v > 127 ? 127 : v);
}

__device__ __forceinline__ uint32_t dq_pack(const float4& v, float inv, float off, int32_t lo) {
  return ((uint32_t)dq_one(v.x, inv, off, lo) & 0xffu) | (((uint32_t)dq_one(v.y, inv, off, lo) & 0xffu) << 8) |
         (((uint32_t)dq_one(v.z, inv, off, lo) & 0xffu) << 16) | (((uint32_t)dq_one(v.w, inv, off, lo) & 0xffu) << 24);
}

}  // namespace bh
