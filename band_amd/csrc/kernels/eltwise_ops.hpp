// Per-element arithmetic of the 8-bit binary ops and the last-axis MEAN,
// shared by the single-op kernels (eltwise_pool.hip, layernorm.hip) so that a
// kernel that strings several ops together performs the very same steps.
#pragma once

#include "common.hpp"

namespace bh {

__device__ __forceinline__ int32_t ld8(const uint8_t* p, long i, bool sgn) {
  return sgn ? (int32_t)(int8_t)p[i] : (int32_t)p[i];
}

__device__ __forceinline__ int32_t elt_op(const bh_eltwise_params& p, int32_t qa, int32_t qb) {
  const int32_t xa = qa + p.a_off;
  const int32_t xb = qb + p.b_off;
  int32_t o;
  if (p.kind == BH_ELT_ADD) {
    const int32_t sa = requant_lt1(xa * (1 << p.left_shift), p.a_mult, p.a_shift);
    const int32_t sb = requant_lt1(xb * (1 << p.left_shift), p.b_mult, p.b_shift);
    o = requant_lt1(sa + sb, p.o_mult, p.o_shift) + p.o_off;
  } else {
    o = requant(xa * xb, p.o_mult, p.o_shift) + p.o_off;
  }
  return clamp_i32(o, p.act_min, p.act_max);
}

// SQUARED_DIFFERENCE int8 (squared_difference.cc, left_shift 7)
__device__ __forceinline__ int32_t sqdiff_op(const bh_eltwise_params& p, int32_t qa, int32_t qb) {
  const int32_t sa = requant_lt1((qa + p.a_off) * (1 << p.left_shift), p.a_mult, p.a_shift);
  const int32_t sb = requant_lt1((qb + p.b_off) * (1 << p.left_shift), p.b_mult, p.b_shift);
  const int32_t d = sa - sb;
  return clamp_i32(requant_lt1(d * d, p.o_mult, p.o_shift) + p.o_off, p.act_min, p.act_max);
}

// the element index of a 4-D operand (a dim of 1 broadcasts) for output index (i0, i1, i2, i3)
__device__ __forceinline__ long bcast_index(const int* s, int i0, int i1, int i2, int i3) {
  return (((long)(s[0] == 1 ? 0 : i0) * s[1] + (s[1] == 1 ? 0 : i1)) * s[2] + (s[2] == 1 ? 0 : i2)) * s[3] +
         (s[3] == 1 ? 0 : i3);
}

// sum of the 4 bytes of a dword, signed or unsigned
__device__ __forceinline__ int32_t sum4(uint32_t w, bool sgn) {
  return sgn ? sbyte(w, 0) + sbyte(w, 1) + sbyte(w, 2) + sbyte(w, 3)
             : (int32_t)((w & 0xff) + ((w >> 8) & 0xff) + ((w >> 16) & 0xff) + (w >> 24));
}

// the sum of all 64 lanes' values, in every lane
__device__ __forceinline__ int32_t wave_sum(int32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// reduce.cc EvalMean over the last axis, from the row's int32 sum: the
// reference_ops::Mean branch (C++ integer division) or QuantizedMeanOrSum's
// float32 sequence, each step rounded on its own (the _rn intrinsics are plain
// operators: the including file is built with -ffp-contract=off)
__device__ __forceinline__ int32_t mean_rows_finish(int32_t sum, int depth, int exact, float scale, float bias,
                                                    int32_t out_zp, bool sgn) {
  if (exact) return sum / depth;
  const float mean = __fdiv_rn((float)sum, (float)depth);
  const int32_t r = (int32_t)roundf(__fadd_rn(__fmul_rn(mean, scale), bias)) + out_zp;
  return sgn ? clamp_i32(r, -128, 127) : clamp_i32(r, 0, 255);
}

}  // namespace bh
