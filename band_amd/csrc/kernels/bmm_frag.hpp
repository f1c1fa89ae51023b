// Fragment loads and LDS staging of the int8 MFMA matmuls (bmm_mfma_kernel in
// batch_matmul.hip, attention_i8_kernel in attention.hip): the 16-byte fragment
// of a K-contiguous operand read from global memory, the staging of a
// K-strided operand's 64 (k) x W block through LDS, and the fragment read of
// the staged image.  batch_matmul.hip's header describes the forms and the
// kBmmPitch bank argument.
#pragma once

#include "common.hpp"
#include "conv_epilogue.hpp"

namespace bh {

constexpr int kBmmPitch = 80;

// 16 K-contiguous bytes of `row` at k .. k + 15, zero past K
template <int VEC>
__device__ __forceinline__ v4i bmm_frag(const uint8_t* row, int k, int K) {
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int u = 0; u < 16 / VEC; ++u) {
    const int kk = k + u * VEC;
    if (kk + VEC <= K) {
      load_unit<VEC>(row + kk, w, u);
    } else if constexpr (VEC > 1) {
#pragma unroll
      for (int b = 0; b < VEC; ++b)
        if (kk + b < K) load_unit<1>(row + kk + b, w, u * VEC + b);
    }
  }
  v4i r;
  r.x = (int)w[0]; r.y = (int)w[1]; r.z = (int)w[2]; r.w = (int)w[3];
  return r;
}

// Stages the 64 (k) x W block of a K-strided operand transposed into `lds`
// (line j = element w0 + j of the contiguous dimension, byte kk = k0 + kk).
// Thread t takes k-row t / 4 and W / 4 consecutive elements; out-of-range
// bytes are written as zero.
template <int W>
__device__ __forceinline__ void bmm_stage(uint8_t* lds, const uint8_t* src, long k_stride, int k0, int K, int w0,
                                          int wlim) {
  const int t = threadIdx.x;
  const int kk = t >> 2;
  const int c0 = (t & 3) * (W / 4);
  const bool krow = k0 + kk < K;
  const uint8_t* g = src + (long)(k0 + kk) * k_stride + w0 + c0;
  const bool vec = (((uintptr_t)src | (uintptr_t)k_stride) & 3) == 0;  // w0, c0 are multiples of 4
#pragma unroll
  for (int d = 0; d < W / 16; ++d) {
    uint32_t v = 0;
    const int w = w0 + c0 + 4 * d;
    if (krow) {
      if (vec && w + 3 < wlim) {
        v = *(const uint32_t*)(g + 4 * d);
      } else {
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (w + b < wlim) v |= (uint32_t)g[4 * d + b] << (8 * b);
      }
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) lds[(c0 + 4 * d + b) * kBmmPitch + kk] = (uint8_t)(v >> (8 * b));
  }
}

// The same block staged as it lies in memory: line kk = k0 + kk, byte j =
// element w0 + j (dword LDS writes); the fragment reads then transpose
// (bmm_lds_frag, TR = 1 / 2).
template <int W>
__device__ __forceinline__ void bmm_stage_rows(uint8_t* lds, const uint8_t* src, long k_stride, int k0, int K, int w0,
                                               int wlim) {
  const int t = threadIdx.x;
  const int kk = t >> 2;
  const int c0 = (t & 3) * (W / 4);
  const bool krow = k0 + kk < K;
  const uint8_t* g = src + (long)(k0 + kk) * k_stride + w0 + c0;
  const bool vec = (((uintptr_t)src | (uintptr_t)k_stride) & 3) == 0;
#pragma unroll
  for (int d = 0; d < W / 16; ++d) {
    uint32_t v = 0;
    const int w = w0 + c0 + 4 * d;
    if (krow) {
      if (vec && w + 3 < wlim) {
        v = *(const uint32_t*)(g + 4 * d);
      } else {
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (w + b < wlim) v |= (uint32_t)g[4 * d + b] << (8 * b);
      }
    }
    *(uint32_t*)(lds + kk * kBmmPitch + c0 + 4 * d) = v;
  }
}

typedef v2i __attribute__((address_space(3))) * lds_v2i_ptr;

// Lane (q, r)'s fragment (k = 16q .. 16q + 15 of element `line + r`) of a
// staged image.
//   TR 0  transposed image (bmm_stage): one ds_read_b128 of line `line + r`.
//   TR 1  row-major image: 16 ds_read_u8 down column `line + r`.
//   TR 2  row-major image: two ds_read_b64_tr_b8.  Within a 16-lane group
//         lane i supplies the address of 8 bytes - row i / 2, byte 8 (i % 2) -
//         of an 8-row x 16-byte block and receives column i of it, row j in
//         byte j; the group of lane quarter q takes rows 16q .. 16q + 7 and
//         16q + 8 .. + 15.  Addresses are multiples of 8 (the pitch is 80,
//         `line` a multiple of 16) and every lane of the wave is active (the
//         caller's branch is wave-uniform).  Banks: a ds_read_b64 is served
//         per 32-lane half over 64 dword banks.  One group's 8 rows start at
//         dwords 20 r' (mod 64: 0, 20, 40, 60, 16, 36, 56, 12), 4 dwords each,
//         disjoint; the half's other group lies 16 rows = 320 dwords = 0 (mod
//         64) further, so odd groups read their upper 8 rows first (+160
//         dwords = 32 mod 64: 32, 52, 8, 28, 48, 4, 24, 44 - disjoint from
//         the even group's) and swap the halves back in registers.
template <int TR>
__device__ __forceinline__ v4i bmm_lds_frag(const uint8_t* img, int line, int r16, int q) {
  if constexpr (TR == 0) {
    return *(const v4i*)(img + (line + r16) * kBmmPitch + 16 * q);
  } else if constexpr (TR == 1) {
    const uint8_t* col = img + 16 * q * kBmmPitch + line + r16;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; ++j) w[j >> 2] |= (uint32_t)col[j * kBmmPitch] << (8 * (j & 3));
    return (v4i){(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
  } else {
    const int sw = q & 1;
    const uint8_t* base = img + (16 * q + (r16 >> 1)) * kBmmPitch + line + 8 * (r16 & 1);
    const v2i r0 = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_v2i_ptr)(base + 8 * kBmmPitch * sw));
    const v2i r1 = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_v2i_ptr)(base + 8 * kBmmPitch * (sw ^ 1)));
    const v2i lo = sw ? r1 : r0, hi = sw ? r0 : r1;
    return (v4i){lo.x, lo.y, hi.x, hi.y};
  }
}

}  // namespace bh
