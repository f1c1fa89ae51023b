// The int8 attention core for gfx950 as one launch: scores = Q K^T (requantised
// to int8), P = SOFTMAX(scores) (int8), out = P V (requantised to int8).  Op by
// op these are bmm_mfma_kernel, softmax_kernel (one thread per row, three byte
// walks of the row in global memory) and bmm_mfma_kernel again, with the scores
// and the probabilities travelling to HBM and back in between.  Here they stay
// in LDS, and operands are taken by strides, so the [B, T, H, D] tensors of a
// converted block are read and written in place of their head TRANSPOSEs.
//
// attention_i8_kernel: a workgroup is 4 waves on 64 query rows of one (b0, b1)
// matrix; wave w owns rows 16 w .. 16 w + 15 of the workgroup's strip from the
// first phase to the last.  The stored bytes are those of the three launches:
// the arithmetic is chan_q / requant_out (conv_epilogue.hpp) on the same
// accumulators and the float sequence of softmax_kernel (glue.hip) on the same
// int8 scores, which is why this file is built with -ffp-contract=off.
//
// Phase 1, Q K^T.  Both operands are K-contiguous (K = head_dim <= 128, two
// K-steps of v_mfma_i32_16x16x64_i8): the wave's Q fragments are loaded once
// and stay in registers, the K fragments of four 16-key tiles at a time come
// straight from global memory (bmm_frag, the widest unit the bases and strides
// allow).  The product is taken transposed as in bmm_mfma_kernel (D^T = K Q^T),
// so lane (q, r) ends with scores [row r][key n0 + 4 q .. + 3]: its four
// requantised bytes are one dword of the LDS strip [64][pitch], pitch =
// roundup(keys, 64) + 16.  The zero-point sums go against the ones fragment.
//
// Phase 2, SOFTMAX of each row in place.  Lane (q, r) of a wave works on row r:
// the four lanes of a row take the row's dwords q, q + 4, ...; the row maximum
// is a max over the lane's dwords and a two-step butterfly (order-free).  The
// row sum is NOT order-free: it is float32, sum = __fadd_rn(sum, table[..])
// over the keys j = 0 .. keys - 1 from 0.0f, as softmax_kernel and the host
// kernel run it, so lane (0, r) walks the row serially (the gathers do not
// depend on the sum, so only the additions form the chain) and hands the sum
// to the row's other lanes.  The output quantisation is per element and uses
// all four lanes again; columns keys .. pitch are written as 0, so that the K
// padding of phase 3 multiplies zeros.
//
// Phase 3, P V with K = keys.  P fragments are ds_read_b128 of the strip (pitch
// / 16 is odd: lane (q, r) reads 16-byte slot r pitch / 16 + q, and r -> r odd
// + q mod 16 is a bijection, the kBmmPitch argument of batch_matmul.hip).  V is
// K-strided: bmm_stage writes each K-step's 64 (k) x out_dim block transposed
// into LDS once for the four waves, which then read their eight (out_dim <=
// 128) column tiles' fragments from it.  The column sums of V are always taken
// (the probabilities' zero point is SOFTMAX's -128), the row sums of P when V's
// zero point is not 0.  The epilogue stores through the output strides, a dword
// per lane where out_dim % 4 == 0 and base and strides are multiples of 4.
//
// The masked form (BIAS, "attention_bias_i8_kernel"): an int8 bias read by
// strides (a padding mask, a causal mask, a position bias) is ADDed to the
// scores in phase 1, between attn_requant4 and the strip: the lane's four bias
// bytes for its row and keys - one dword, four bytes or one byte replicated,
// clamped to the last row and key like the Q and K reads - are loaded ahead of
// the round's MFMAs and meet the four score bytes in TFLite's int8 ADD
// (residual_add.hpp, the direct form: no table, no LDS, no barrier of its
// own).  Phases 2 and 3 do not know of it; the stored bytes are those of the
// four launches with bh_eltwise_i8 (BH_ELT_ADD) between the first two.
//
// LDS: the strip (64 pitch), V's staging (128 lines of kBmmPitch) and the exp
// table (1 KB), sized per launch: 11 KB + 64 pitch, i.e. 28 KB at keys 196 and
// 76 KB at keys 1024 (BH_ATTENTION_MAX_KEYS), above 64 KB with the dynamic-LDS
// attribute set once per process and device.
#include <climits>
#include <type_traits>

#include "band_hip_attention_shared.h"
#include "bmm_frag.hpp"
#include "common.hpp"
#include "conv_epilogue.hpp"
#include "residual_add.hpp"

namespace bh {

constexpr int kAttnRows = 64;       // query rows per workgroup
constexpr int kAttnTiles = 4;       // key tiles per phase-1 round
constexpr int kAttnStageBytes = BH_ATTENTION_MAX_DIM * kBmmPitch;

__host__ __device__ inline int attn_pitch(int keys) { return (keys + 63) / 64 * 64 + 16; }

template <bool FAST>
__device__ __forceinline__ uint32_t attn_requant4(v4i acc, v4i rs, v4i cs, const bh_attention_quant& z, int32_t kzz,
                                                  const ChanQ& cq) {
  uint32_t packed = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int32_t s = acc[r] - z.rhs_zp * rs[r] - z.lhs_zp * cs[r] + kzz;
    const int32_t v = requant_out<FAST>(s, cq, z.out_zp, -128, 127);
    packed |= ((uint32_t)v & 0xffu) << (8 * r);
  }
  return packed;
}

// bh_attention_params as the kernel takes it: strides in 32 bits (every index
// is below 2^31 by the launcher's check; the stride of an extent of 1 is 0)
struct AttnArgs {
  int32_t rows, keys, head_dim, out_dim;
  int32_t q_bstride[2], k_bstride[2], v_bstride[2], out_bstride[2];
  int32_t q_row_stride, k_row_stride, v_row_stride, out_row_stride;
  bh_attention_quant qk, pv;
  float sm_out_scale;
  int32_t sm_out_zp;
  int32_t fast;  // bit 0 / 1: single-step requantisation of Q K^T / P V
  const float* table;
  const void* q;
  const void* k;
  const void* v;
  void* out;
};

// the masked form's arguments: the bias by strides (0 broadcasts) and the ADD's constants
struct AttnBiasArgs : AttnArgs {
  const void* bias;
  int32_t bias_bstride[2], bias_row_stride, bias_key_stride;
  int32_t bias_vec4;  // dword loads: key stride 1, keys % 4 == 0, base and strides multiples of 4
  int32_t add_scores_operand;
  bh_attention_add add;
};

// the lane's four bias bytes for keys kb .. kb + 3 of its row, clamped to the last key as the K reads are
__device__ __forceinline__ uint32_t attn_bias4(const AttnBiasArgs& p, const uint8_t* brow, int kb, int keys) {
  if (p.bias_key_stride == 0) return splat_byte(brow[0]);
  if (p.bias_vec4) return *(const uint32_t*)(brow + min(kb, keys - 4));
  uint32_t w = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) w |= (uint32_t)brow[min(kb + r, keys - 1)] << (8 * r);
  return w;
}

// ADD(score, bias) on the four bytes of a lane's dword
__device__ __forceinline__ uint32_t attn_add4(const ResidualAdd& A, uint32_t scores, uint32_t bias) {
  uint32_t packed = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    packed |= ((uint32_t)residual_add(A, sbyte(scores, r), sbyte(bias, r)) & 0xffu) << (8 * r);
  return packed;
}

// VEC: fragment unit of Q and K; BIAS: the masked form, ADD(scores, bias) between the first product's
// requantisation and the strip ("attention_bias_i8_kernel" in launch lists)
template <int VEC, bool BIAS>
__global__ __launch_bounds__(256) void attention_i8_kernel(std::conditional_t<BIAS, AttnBiasArgs, AttnArgs> p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int keys = p.keys, D = p.head_dim, N = p.out_dim, M = p.rows;
  const int pitch = attn_pitch(keys);
  uint8_t* strip = smem;
  uint8_t* ldsV = smem + kAttnRows * pitch;
  float* tab = (float*)(ldsV + kAttnStageBytes);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int r16 = lane & 15;
  const int q = lane >> 4;
  const int b1 = blockIdx.y, b0 = blockIdx.z;
  const int m0 = (int)blockIdx.x * kAttnRows + wave * 16;
  const bool active = m0 < M;  // whole wave; an idle wave still stages V and meets the barriers
  const uint8_t* Q = (const uint8_t*)p.q + (long)b0 * p.q_bstride[0] + (long)b1 * p.q_bstride[1];
  const uint8_t* Kp = (const uint8_t*)p.k + (long)b0 * p.k_bstride[0] + (long)b1 * p.k_bstride[1];
  const uint8_t* V = (const uint8_t*)p.v + (long)b0 * p.v_bstride[0] + (long)b1 * p.v_bstride[1];
  const v4i ones = (v4i){0x01010101, 0x01010101, 0x01010101, 0x01010101};
  const v4i zero = (v4i){0, 0, 0, 0};
  uint8_t* myrow = strip + (wave * 16 + r16) * pitch;

  tab[threadIdx.x] = p.table[threadIdx.x];

  // ---- phase 1: scores into the strip -------------------------------------------------
  if (active) {
    // this lane's query row, clamped: rows past M are computed and never stored
    const uint8_t* qrow = Q + (long)min(m0 + r16, M - 1) * p.q_row_stride;
    const bool two = D > 64;
    const v4i a0 = bmm_frag<VEC>(qrow, 16 * q, D);
    const v4i a1 = two ? bmm_frag<VEC>(qrow, 64 + 16 * q, D) : zero;
    const bool need_rs = p.qk.rhs_zp != 0;  // z_r sum_k q[i, k]
    const bool need_cs = p.qk.lhs_zp != 0;  // z_l sum_k k[j, k]
    v4i rs = zero;
    if (need_rs) {
      rs = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, a0, rs, 0, 0, 0);
      if (two) rs = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, a1, rs, 0, 0, 0);
    }
    const int32_t kzz = D * p.qk.lhs_zp * p.qk.rhs_zp;
    const ChanQ cq = chan_q(p.qk.mult, p.qk.shift, p.qk.out_zp);
    const uint8_t* brow = nullptr;
    if constexpr (BIAS)
      brow = (const uint8_t*)p.bias + (long)b0 * p.bias_bstride[0] + (long)b1 * p.bias_bstride[1] +
             (long)min(m0 + r16, M - 1) * p.bias_row_stride;
    for (int n0 = 0; n0 < keys; n0 += 16 * kAttnTiles) {
      v4i acc[kAttnTiles], cs[kAttnTiles];
      uint32_t bw[kAttnTiles];
      if constexpr (BIAS) {
        // issued ahead of the round's K loads and MFMAs, met after them
#pragma unroll
        for (int t = 0; t < kAttnTiles; ++t)
          bw[t] = n0 + 16 * t < keys ? attn_bias4(p, brow, n0 + 16 * t + 4 * q, keys) : 0u;
      }
#pragma unroll
      for (int t = 0; t < kAttnTiles; ++t) {
        acc[t] = zero;
        cs[t] = zero;
        if (n0 + 16 * t >= keys) continue;  // whole wave
        const uint8_t* kcol = Kp + (long)min(n0 + 16 * t + r16, keys - 1) * p.k_row_stride;
        const v4i b = bmm_frag<VEC>(kcol, 16 * q, D);
        acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(b, a0, acc[t], 0, 0, 0);
        if (need_cs) cs[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(b, ones, cs[t], 0, 0, 0);
        if (two) {
          const v4i b2 = bmm_frag<VEC>(kcol, 64 + 16 * q, D);
          acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(b2, a1, acc[t], 0, 0, 0);
          if (need_cs) cs[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(b2, ones, cs[t], 0, 0, 0);
        }
      }
#pragma unroll
      for (int t = 0; t < kAttnTiles; ++t) {
        if (n0 + 16 * t >= keys) continue;
        // keys past `keys` in the last tile hold a clamped column's score: phase 2 overwrites them with 0
        uint32_t s4 = (p.fast & 1) ? attn_requant4<true>(acc[t], rs, cs[t], p.qk, kzz, cq)
                                   : attn_requant4<false>(acc[t], rs, cs[t], p.qk, kzz, cq);
        if constexpr (BIAS) s4 = attn_add4(residual_of(p.add, p.add_scores_operand), s4, bw[t]);
        *(uint32_t*)(myrow + n0 + 16 * t + 4 * q) = s4;
      }
    }
  }
  __syncthreads();  // the strip's rows (written by lanes (q, r), read by lanes (q', r)) and the table

  // ---- phase 2: softmax of row r16 in place ------------------------------------------
  if (active) {
    const int nd = (keys + 3) >> 2;  // dwords holding scores
    const uint32_t* rw = (const uint32_t*)myrow;
    int32_t mx = -128;
    for (int d = q; d < nd; d += 4) {
      const uint32_t w = rw[d];
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (4 * d + b < keys) mx = max(mx, sbyte(w, b));
    }
    mx = max(mx, __shfl_xor(mx, 16));
    mx = max(mx, __shfl_xor(mx, 32));
    const float* to = tab + 255 - mx;
    float sum = 0.0f;
    if (q == 0) {
      for (int d = 0; d < nd; ++d) {
        const uint32_t w = rw[d];
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (4 * d + b < keys) sum = __fadd_rn(sum, to[sbyte(w, b)]);
      }
    }
    sum = __shfl(sum, r16);
    const float inv = __fdiv_rn(1.0f, __fmul_rn(sum, p.sm_out_scale));
    for (int d = q; d < pitch / 4; d += 4) {
      uint32_t o = 0;
      if (d < nd) {
        const uint32_t w = rw[d];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          if (4 * d + b >= keys) continue;
          const float pr = __fmul_rn(to[sbyte(w, b)], inv);
          const int32_t v = clamp_i32((int32_t)roundf(pr) + p.sm_out_zp, -128, 127);
          o |= ((uint32_t)v & 0xffu) << (8 * b);
        }
      }
      ((uint32_t*)myrow)[d] = o;
    }
  }

  // ---- phase 3: P V -------------------------------------------------------------------
  constexpr int kNT = BH_ATTENTION_MAX_DIM / 16;
  v4i acc[kNT], cs[kNT], rs = zero;
#pragma unroll
  for (int t = 0; t < kNT; ++t) {
    acc[t] = zero;
    cs[t] = zero;
  }
  const bool need_rs = p.pv.rhs_zp != 0;  // z_r sum_k p[i, k]
  for (int k0 = 0; k0 < keys; k0 += 64) {
    __syncthreads();  // the previous step's fragment reads; before the first step, phase 2's strip writes
    bmm_stage<64>(ldsV, V, p.v_row_stride, k0, keys, 0, N);
    if (N > 64) bmm_stage<64>(ldsV + 64 * kBmmPitch, V, p.v_row_stride, k0, keys, 64, N);
    __syncthreads();
    if (active) {
      const v4i a = *(const v4i*)(myrow + k0 + 16 * q);
      if (need_rs) rs = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, a, rs, 0, 0, 0);
#pragma unroll
      for (int t = 0; t < kNT; ++t) {
        if (16 * t >= N) break;  // whole workgroup
        const v4i b = bmm_lds_frag<0>(ldsV, 16 * t, r16, q);
        acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(b, a, acc[t], 0, 0, 0);
        cs[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(b, ones, cs[t], 0, 0, 0);
      }
    }
  }

  const int m = m0 + r16;
  if (!active || m >= M) return;
  const int32_t kzz = keys * p.pv.lhs_zp * p.pv.rhs_zp;
  const ChanQ cq = chan_q(p.pv.mult, p.pv.shift, p.pv.out_zp);
  const bool vec_store = (N & 3) == 0 && (((uintptr_t)p.out | (uintptr_t)p.out_row_stride | (uintptr_t)p.out_bstride[0] |
                                           (uintptr_t)p.out_bstride[1]) & 3) == 0;  // (a stride of 0 stands for an extent of 1)
  uint8_t* orow = (uint8_t*)p.out + (long)b0 * p.out_bstride[0] + (long)b1 * p.out_bstride[1] + (long)m * p.out_row_stride;
#pragma unroll
  for (int t = 0; t < kNT; ++t) {
    const int nb = 16 * t + 4 * q;
    if (nb >= N) break;  // later tiles start further right
    const uint32_t packed = (p.fast & 2) ? attn_requant4<true>(acc[t], rs, cs[t], p.pv, kzz, cq)
                                       : attn_requant4<false>(acc[t], rs, cs[t], p.pv, kzz, cq);
    uint8_t* out = orow + nb;
    if (vec_store) {
      *(uint32_t*)out = packed;
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (nb + r < N) out[r] = (uint8_t)(packed >> (8 * r));
    }
  }
}

// nullptr = runnable (band_hip_attention_shared.h: host code, also run under sanitizers on its own)
static const char* attn_check(const bh_attention_params* p) { return bh_attention_why(p); }
static_assert(kAttnRows == BH_ATTENTION_ROWS, "the check's rows per workgroup");

static size_t attn_lds_bytes(int keys) { return (size_t)kAttnRows * attn_pitch(keys) + kAttnStageBytes + 256 * sizeof(float); }
static_assert(kAttnRows * (BH_ATTENTION_MAX_KEYS + 16) + kAttnStageBytes + 1024 <= 160 * 1024,
              "the largest strip must fit the CU's LDS");

template <int VEC, bool BIAS>
static void attn_launch(const bh_attention_params& p, int fast, hipStream_t s) {
  const size_t lds = attn_lds_bytes(p.keys);
  if (lds > 64 * 1024) {
    static thread_local int opted_device = -1;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (opted_device != dev) {
      (void)hipFuncSetAttribute((const void*)attention_i8_kernel<VEC, BIAS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                160 * 1024);
      opted_device = dev;
    }
  }
  const dim3 grid((unsigned)((p.rows + kAttnRows - 1) / kAttnRows), (unsigned)p.batch[1], (unsigned)p.batch[0]);
  std::conditional_t<BIAS, AttnBiasArgs, AttnArgs> a{};
  a.rows = p.rows; a.keys = p.keys; a.head_dim = p.head_dim; a.out_dim = p.out_dim;
  for (int d = 0; d < 2; ++d) {
    const bool walk = p.batch[d] > 1;
    a.q_bstride[d] = walk ? (int32_t)p.q_bstride[d] : 0;
    a.k_bstride[d] = walk ? (int32_t)p.k_bstride[d] : 0;
    a.v_bstride[d] = walk ? (int32_t)p.v_bstride[d] : 0;
    a.out_bstride[d] = walk ? (int32_t)p.out_bstride[d] : 0;
  }
  a.q_row_stride = p.rows > 1 ? (int32_t)p.q_row_stride : 0;
  a.k_row_stride = p.keys > 1 ? (int32_t)p.k_row_stride : 0;
  a.v_row_stride = p.keys > 1 ? (int32_t)p.v_row_stride : 0;
  a.out_row_stride = p.rows > 1 ? (int32_t)p.out_row_stride : 0;
  a.qk = p.qk; a.pv = p.pv;
  a.sm_out_scale = p.sm_out_scale; a.sm_out_zp = p.sm_out_zp; a.fast = fast;
  a.table = p.table; a.q = p.q; a.k = p.k; a.v = p.v; a.out = p.out;
  if constexpr (BIAS) {
    a.bias = p.bias;
    for (int d = 0; d < 2; ++d) a.bias_bstride[d] = p.batch[d] > 1 ? (int32_t)p.bias_bstride[d] : 0;
    a.bias_row_stride = p.rows > 1 ? (int32_t)p.bias_row_stride : 0;
    a.bias_key_stride = p.keys > 1 ? (int32_t)p.bias_key_stride : 0;
    // a dword per lane and tile: keys % 4 == 0 keeps the clamped last dword inside the row
    const uintptr_t al = (uintptr_t)p.bias | (uintptr_t)a.bias_bstride[0] | (uintptr_t)a.bias_bstride[1] |
                         (uintptr_t)a.bias_row_stride | (uintptr_t)p.keys;
    a.bias_vec4 = a.bias_key_stride == 1 && al % 4 == 0 && !(p.kernel_hint & BH_ATTN_BYTES);
    a.add_scores_operand = p.add_scores_operand;
    a.add = p.add;
  }
  BH_LAUNCH((attention_i8_kernel<VEC, BIAS>), grid, dim3(256), lds, s, a);
}

template <bool BIAS>
static void attn_launch_vec(const bh_attention_params& p, int vec, int fast, hipStream_t s) {
  if (vec == 16) attn_launch<16, BIAS>(p, fast, s);
  else if (vec == 8) attn_launch<8, BIAS>(p, fast, s);
  else if (vec == 4) attn_launch<4, BIAS>(p, fast, s);
  else attn_launch<1, BIAS>(p, fast, s);
}

}  // namespace bh

extern "C" int bh_attention_i8_check(const bh_attention_params* p) {
  const char* why = bh::attn_check(p);
  if (!why) return 0;
  static thread_local char msg[160];
  snprintf(msg, sizeof(msg), "bh_attention_i8: %s", why);
  bh_set_last_error(msg);
  return BH_EINVAL;
}

extern "C" const char* bh_attention_i8_kernel(const bh_attention_params* p) {
  return bh::attn_check(p) ? "" : (p->bias ? "attention_bias_i8_kernel" : "attention_i8_kernel");
}

extern "C" size_t bh_attention_i8_lds_bytes(const bh_attention_params* p) {
  return bh::attn_check(p) ? 0 : bh::attn_lds_bytes(p->keys);
}

extern "C" int bh_attention_i8(const bh_attention_params* pp, bh_stream_t stream) {
  using namespace bh;
  if (bh_attention_i8_check(pp) != 0) return BH_EINVAL;
  const bh_attention_params& p = *pp;
  // widest fragment unit of Q and K: their bases and their row and batch strides decide
  const uintptr_t al = (uintptr_t)p.q | (uintptr_t)p.q_row_stride | (uintptr_t)p.q_bstride[0] | (uintptr_t)p.q_bstride[1] |
                       (uintptr_t)p.k | (uintptr_t)p.k_row_stride | (uintptr_t)p.k_bstride[0] | (uintptr_t)p.k_bstride[1];
  int vec = al % 16 == 0 ? 16 : (al % 8 == 0 ? 8 : (al % 4 == 0 ? 4 : 1));
  if (p.kernel_hint & BH_ATTN_BYTES) vec = 1;
  // single-step requantisation per product, as bh_batch_matmul_i8 decides it
  const int fast = (p.qk.requant_fast != 0 && bh_conv_requant_fast_ok(&p.qk.mult, &p.qk.shift, 1, p.head_dim, 0) ? 1 : 0) |
                   (p.pv.requant_fast != 0 && bh_conv_requant_fast_ok(&p.pv.mult, &p.pv.shift, 1, p.keys, 0) ? 2 : 0);
  hipStream_t s = (hipStream_t)stream;
  if (p.bias) attn_launch_vec<true>(p, vec, fast, s);
  else attn_launch_vec<false>(p, vec, fast, s);
  return bh_check_launch(p.bias ? "attention_bias_i8_kernel" : "attention_i8_kernel");
}
