// Pieces of the int8 CONV_2D kernels shared by conv_mfma.hip and
// conv_grouped.hip: the row descriptor and fragment-unit loads of the im2col
// gathers and the transposed-tile epilogue (requantisation, residual ADD, byte table, the
// 4-channel dword store).
#pragma once

#include "common.hpp"
#include "residual_add.hpp"

namespace bh {

struct RowInfo {
  long base;   // 1x1: byte offset of the input pixel; general: image base
  int y0, x0;  // general: top-left input coordinate of the window
  bool valid;
};

template <int VEC>
__device__ __forceinline__ void load_unit(const uint8_t* src, uint32_t* w, int u) {
  if constexpr (VEC == 16) {
    v4i v = *(const v4i*)src;
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  } else if constexpr (VEC == 8) {
    v2i v = *(const v2i*)src;
    w[2 * u] = v.x; w[2 * u + 1] = v.y;
  } else if constexpr (VEC == 4) {
    w[u] = *(const uint32_t*)src;
  } else {
    const int d = u >> 2, b = u & 3;
    w[d] = (w[d] & ~(0xffu << (8 * b))) | ((uint32_t)src[0] << (8 * b));
  }
}

template <int VEC>
__device__ __forceinline__ void xor_unit(uint32_t* w, int u, uint32_t xorw) {
  if constexpr (VEC == 16) {
    w[0] ^= xorw; w[1] ^= xorw; w[2] ^= xorw; w[3] ^= xorw;
  } else if constexpr (VEC == 8) {
    w[2 * u] ^= xorw; w[2 * u + 1] ^= xorw;
  } else if constexpr (VEC == 4) {
    w[u] ^= xorw;
  } else {
    const int d = u >> 2, b = u & 3;
    w[d] ^= (xorw & (0xffu << (8 * b)));
  }
}

template <int VEC>
__device__ __forceinline__ void fill_unit(uint32_t* w, int u, uint32_t pat) {
  if constexpr (VEC == 16) {
    w[0] = w[1] = w[2] = w[3] = pat;
  } else if constexpr (VEC == 8) {
    w[2 * u] = pat; w[2 * u + 1] = pat;
  } else if constexpr (VEC == 4) {
    w[u] = pat;
  } else {
    const int d = u >> 2, b = u & 3;
    w[d] = (w[d] & ~(0xffu << (8 * b))) | ((pat & 0xffu) << (8 * b));
  }
}

// Per-lane channel constants of a transposed 16x16 tile's epilogue: the lane
// owns output channels nb..nb+3 (every pixel row of the tile uses the same
// four), so kernels that store several pixel tiles per channel group build
// them once.
struct Chan4 {
  int32_t be[4];
  ChanQ q[4];
  bool vec;  // dword path: N % 4 == 0 and 4-byte aligned output / residual bases
};

__device__ __forceinline__ Chan4 chan4(const bh_conv_params& p, int nb, int N) {
  Chan4 c;
  // (a concat-elided output may start at any byte, and its images at any
  // stride)
  c.vec = (N & 3) == 0 && (((uintptr_t)p.output | (uintptr_t)p.residual | (uintptr_t)p.out_img_stride) & 3) == 0;
  int32_t mu[4], sh[4];
  if (c.vec) {
    const v4i b4 = *(const v4i*)(p.bias_eff + nb);
    const v4i m4 = *(const v4i*)(p.mult + nb);
    const v4i s4 = *(const v4i*)(p.shift + nb);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      c.be[r] = b4[r];
      mu[r] = m4[r];
      sh[r] = s4[r];
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = nb + r < N ? nb + r : nb;
      c.be[r] = p.bias_eff[n];
      mu[r] = p.mult[n];
      sh[r] = p.shift[n];
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) c.q[r] = chan_q(mu[r], sh[r], p.out_zp);
  return c;
}

// Epilogue of one transposed 16x16 tile: the lane holds output channels
// nb..nb+3 of pixel m (D^T = W x X^T on the MFMA), so its four requantised
// bytes leave as one dword store when N % 4 == 0.  acc excludes the folded
// bias; rsum is pixel m's input row sum (uint8 filters).
__device__ __forceinline__ void conv_store4(const bh_conv_params& p, v4i acc, int rsum, int m, int nb, int M, int N,
                                            const Chan4& c) {
  if (m >= M || nb >= N) return;
  const long o = (long)m * N + nb;
  const uint8_t* res = (const uint8_t*)p.residual;
  const bool res_signed = p.in_xor == 0;  // residual shares the activation type
  const uint8_t* tab = (const uint8_t*)p.out_table;
  uint32_t rq = 0;
  if (res) {
    if (c.vec) {
      rq = *(const uint32_t*)(res + o);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (nb + r < N) rq |= (uint32_t)res[o + r] << (8 * r);
    }
  }
  const ResidualAdd A = residual_of(p);
  uint32_t packed = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int32_t a = acc[r] + c.be[r];
    if (p.w_zp != 0) a -= p.w_zp * rsum;
    int32_t v = p.requant_fast ? requant_out<true>(a, c.q[r], p.out_zp, p.act_min, p.act_max)
                               : requant_out<false>(a, c.q[r], p.out_zp, p.act_min, p.act_max);
    if (res) v = residual_add(A, v, residual_byte(rq, r, res_signed));
    const uint32_t byte = tab ? tab[(uint8_t)v] : ((uint32_t)v & 0xffu);
    packed |= byte << (8 * r);
  }
  long oo = o;
  if (p.out_img_stride) {  // a slice of a concatenation: image n at n * stride (uniform branch)
    const int hw = p.out_h * p.out_w;
    const int img = m / hw;
    oo = (long)img * p.out_img_stride + (long)(m - img * hw) * N + nb;
  }
  uint8_t* out = (uint8_t*)p.output + oo;
  if (c.vec) {
    *(uint32_t*)out = packed;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (nb + r < N) out[r] = (uint8_t)(packed >> (8 * r));
  }
}

__device__ __forceinline__ void conv_epilogue4(const bh_conv_params& p, v4i acc, int rsum, int m, int nb, int M,
                                               int N) {
  if (m >= M || nb >= N) return;
  conv_store4(p, acc, rsum, m, nb, M, N, chan4(p, nb, N));
}

}  // namespace bh
