// Dynamic-range ("hybrid") CONV_2D and DEPTHWISE_CONV_2D for gfx950: float32
// activations, a constant int8 filter with zero points 0, each batch item
// quantised to int8 at run time, an int8 product, a float32 epilogue.
// Restated from memory of TFLite's conv.cc EvalHybrid / EvalHybridPerChannel
// and depthwise_conv.cc EvalHybridPerChannel; band_hip_kernels.h and DESIGN 4
// hold the rule and say what is pinned.
//
// Quantisation (bh_dynquant_items): the row rule of dynquant_rows_kernel
// (dynquant.hpp) with a whole item - H W C floats - as the row.  A 112 x 112 x
// 96 item is far too long for one wave, so an item is spread over workgroups
// of 256 threads, one per chunk of BH_DYNQUANT_CHUNK floats:
//   dynquant_minmax_kernel  a (min, max) pair per chunk, stored as one float2
//   dynquant_items_kernel   every workgroup reduces its item's pairs (min and
//                           max are exact in any order), derives (s, inv, off)
//                           and quantises its own chunk; chunk 0 stores s, off
// or, for an item of a few chunks, dynquant_item_kernel: one workgroup per
// item runs both passes in one launch.  Items whose floats are 16-byte aligned
// are read as float4 and stored as dwords, anything else element by element.
//
// conv_hybrid_kernel: the implicit-im2col GEMM M = batch out_h out_w,
// N = out_c, K = k_h k_w in_c on v_mfma_i32_16x16x64_i8, unstaged as
// fc_hybrid_kernel is: the filter is packed [out_c][k_pad] with zero padding so
// its fragments are whole 16-byte loads, the activation fragment is gathered
// (VEC = 16: in_c a multiple of 16, a fragment lies inside one tap and is one
// load; 4: dword units; 1: bytes), a padded tap reads as the byte off[b] of the
// row's own item (a 16-row tile may span items), the K tail as zero.  A wave
// takes 16 rows x NT 16-channel tiles (NT = 4 on the large layers, 1 where
// that would leave the machine short of workgroups), a workgroup's 4 waves 4
// adjacent row tiles; a small layer with a deep K (the 14 x 14 and 7 x 7
// layers, the classifier head) gives a workgroup one 16-row tile instead, the
// waves split the K-steps and the partial sums meet in LDS as int32
// (conv_hybrid_form).
//   acc' = acc - off[b] * w_row_sum[c]            (the rule's in-bounds sum)
//   per_channel 0:  y = bias[c] + (float)acc' * (s[b] * ws[c])
//   per_channel 1:  y = ((float)acc' * ws[c]) * s[b] + bias[c]
//
// dwconv_hybrid_kernel: VALU over NHWC, a lane per 4 consecutive output
// channels of a pixel; in-bounds taps only, int8 x int8 into int32 with the
// taps' filter sum beside it:  y = (float)(acc - off[b] wsum) * (ws[c] * s[b])
// + bias[c].  Dword reads of taps and filter where depth_multiplier == 1 and
// the channel count is a multiple of 4.
// No atomics, no scratch.
#include <climits>

#include "common.hpp"
#include "dynquant.hpp"

namespace bh {

constexpr int kDqBlock = 256;

// the workgroup's min / max from every thread's; sm holds 8 floats
__device__ __forceinline__ void block_minmax(float& mn, float& mx, float* sm) {
  mn = wave_min(mn);
  mx = wave_max(mx);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sm[wave] = mn;
    sm[4 + wave] = mx;
  }
  __syncthreads();
  mn = fminf(fminf(sm[0], sm[1]), fminf(sm[2], sm[3]));
  mx = fmaxf(fmaxf(sm[4], sm[5]), fmaxf(sm[6], sm[7]));
}

template <bool VEC4>
__device__ __forceinline__ void span_minmax(const float* x, int n, float& mn, float& mx) {
  if constexpr (VEC4) {
    for (int i = threadIdx.x; i < (n >> 2); i += kDqBlock) {
      const float4 v = ((const float4*)x)[i];
      mn = fminf(mn, fminf(fminf(v.x, v.y), fminf(v.z, v.w)));
      mx = fmaxf(mx, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
    }
  } else {
    for (int i = threadIdx.x; i < n; i += kDqBlock) {
      mn = fminf(mn, x[i]);
      mx = fmaxf(mx, x[i]);
    }
  }
}

template <bool VEC4>
__device__ __forceinline__ void span_quant(const float* x, int8_t* q, int n, float inv, float foff, int32_t lo) {
  if constexpr (VEC4) {
    for (int i = threadIdx.x; i < (n >> 2); i += kDqBlock) ((uint32_t*)q)[i] = dq_pack(((const float4*)x)[i], inv, foff, lo);
  } else {
    for (int i = threadIdx.x; i < n; i += kDqBlock) q[i] = (int8_t)dq_one(x[i], inv, foff, lo);
  }
}

// lane 0 of each wave derives, the wave shares: dynquant_rows_kernel's sequence
__device__ __forceinline__ void derive_shared(float mn, float mx, bool asym, float& s, float& inv, int32_t& off) {
  s = 1.f;
  inv = 0.f;
  off = 0;
  if ((threadIdx.x & 63) == 0) dq_derive(mn, mx, asym, s, inv, off);
  s = __shfl(s, 0);
  inv = __shfl(inv, 0);
  off = __shfl(off, 0);
}

template <bool VEC4>
__global__ __launch_bounds__(kDqBlock) void dynquant_item_kernel(bh_dynquant_items_params p) {
  __shared__ float sm[8];
  const long base = (long)blockIdx.x * p.item_size;
  const float* x = p.input + base;
  float mn = 0.f, mx = 0.f;
  span_minmax<VEC4>(x, p.item_size, mn, mx);
  block_minmax(mn, mx, sm);
  float s, inv;
  int32_t off;
  derive_shared(mn, mx, p.asymmetric != 0, s, inv, off);
  if (threadIdx.x == 0) {
    p.scale[blockIdx.x] = s;
    p.offset[blockIdx.x] = off;
  }
  span_quant<VEC4>(x, p.q + base, p.item_size, inv, (float)off, p.asymmetric ? -128 : -127);
}

template <bool VEC4>
__global__ __launch_bounds__(kDqBlock) void dynquant_minmax_kernel(bh_dynquant_items_params p, FastDiv chunks) {
  __shared__ float sm[8];
  const int item = (int)chunks.div(blockIdx.x);
  const int chunk = (int)blockIdx.x - item * (int)chunks.d;
  const int first = chunk * BH_DYNQUANT_CHUNK;
  const int n = min(BH_DYNQUANT_CHUNK, p.item_size - first);
  float mn = 0.f, mx = 0.f;
  span_minmax<VEC4>(p.input + (long)item * p.item_size + first, n, mn, mx);
  block_minmax(mn, mx, sm);
  if (threadIdx.x == 0) ((float2*)p.pairs)[blockIdx.x] = make_float2(mn, mx);
}

template <bool VEC4>
__global__ __launch_bounds__(kDqBlock) void dynquant_items_kernel(bh_dynquant_items_params p, FastDiv chunks) {
  __shared__ float sm[8];
  const int item = (int)chunks.div(blockIdx.x);
  const int chunk = (int)blockIdx.x - item * (int)chunks.d;
  const float2* pairs = (const float2*)p.pairs + (long)item * chunks.d;
  float mn = 0.f, mx = 0.f;
  for (int c = threadIdx.x; c < (int)chunks.d; c += kDqBlock) {
    const float2 v = pairs[c];
    mn = fminf(mn, v.x);
    mx = fmaxf(mx, v.y);
  }
  block_minmax(mn, mx, sm);
  float s, inv;
  int32_t off;
  derive_shared(mn, mx, p.asymmetric != 0, s, inv, off);
  if (chunk == 0 && threadIdx.x == 0) {
    p.scale[item] = s;
    p.offset[item] = off;
  }
  const int first = chunk * BH_DYNQUANT_CHUNK;
  const int n = min(BH_DYNQUANT_CHUNK, p.item_size - first);
  const long base = (long)item * p.item_size + first;
  span_quant<VEC4>(p.input + base, p.q + base, n, inv, (float)off, p.asymmetric ? -128 : -127);
}

// ---- conv_hybrid_kernel ----------------------------------------------------------------

struct ConvHyDivs {
  FastDiv out_w, out_hw, in_c, k_w;
};

enum ConvHybridForm { kHyTiles = 0, kHySplit = 1 };

// 16 bytes of row (iy0, ix0)'s im2col line at k .. k + 15: an out-of-bounds tap
// reads as `padb`, bytes past K as zero
template <int VEC>
__device__ __forceinline__ v4i conv_hybrid_frag(const uint8_t* img, int k, int K, int iy0, int ix0, uint32_t padb,
                                                const bh_conv_hybrid_params& p, const ConvHyDivs& dv) {
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  if (k < K) {
    const int tap = (int)dv.in_c.div((uint32_t)k);
    int ci = k - tap * p.in_c;
    int ky = (int)dv.k_w.div((uint32_t)tap);
    int kx = tap - ky * p.k_w;
#pragma unroll
    for (int u = 0; u < 16 / VEC; ++u) {
      if (k + u * VEC < K) {  // in_c % VEC == 0: a unit is whole or absent
        const int iy = iy0 + ky * p.dil_h, ix = ix0 + kx * p.dil_w;
        const bool inb = (unsigned)iy < (unsigned)p.in_h && (unsigned)ix < (unsigned)p.in_w;
        const uint8_t* src = img + ((long)iy * p.in_w + ix) * p.in_c + ci;
        if constexpr (VEC == 16) {
          if (inb) {
            const v4i v = *(const v4i*)src;
            w[0] = (uint32_t)v.x; w[1] = (uint32_t)v.y; w[2] = (uint32_t)v.z; w[3] = (uint32_t)v.w;
          } else {
            w[0] = w[1] = w[2] = w[3] = padb * 0x01010101u;
          }
        } else if constexpr (VEC == 4) {
          w[u] = inb ? *(const uint32_t*)src : padb * 0x01010101u;
        } else {
          w[u >> 2] |= (inb ? (uint32_t)*src : padb) << (8 * (u & 3));
        }
        ci += VEC;
        if (ci >= p.in_c) {
          ci = 0;
          if (++kx == p.k_w) {
            kx = 0;
            ++ky;
          }
        }
      }
    }
  }
  return (v4i){(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
}

template <int VEC, int FORM, int NT>
__global__ __launch_bounds__(256) void conv_hybrid_kernel(bh_conv_hybrid_params p, ConvHyDivs dv, int gn) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int r16 = lane & 15;
  const int q = lane >> 4;
  const int M = p.batch * p.out_h * p.out_w, N = p.out_c, K = p.k_h * p.k_w * p.in_c, KP = p.k_pad;
  // channel blocks fastest: neighbouring workgroups gather the same rows
  const int bm = (int)blockIdx.x / gn;
  const int n0 = ((int)blockIdx.x - bm * gn) * (16 * NT);
  const int m0 = FORM == kHyTiles ? bm * 64 + wave * 16 : bm * 16;
  const bool active = m0 < M;  // whole wave; n0 < N by the grid
  const int nt = min(NT, (N - n0 + 15) >> 4);
  // this lane's row, clamped: results of the clamped rows are never stored
  const int mrow = min(m0 + r16, M - 1);
  const int b = (int)dv.out_hw.div((uint32_t)mrow);
  const int rem = mrow - b * (int)dv.out_hw.d;
  const int oy = (int)dv.out_w.div((uint32_t)rem);
  const int ox = rem - oy * p.out_w;
  const int iy0 = oy * p.stride_h - p.pad_h, ix0 = ox * p.stride_w - p.pad_w;
  const uint8_t* img = (const uint8_t*)p.q + (long)b * p.in_h * p.in_w * p.in_c;
  const int32_t off = p.in_offset[b];
  const uint32_t padb = (uint32_t)off & 0xffu;
  const uint8_t* wbase = (const uint8_t*)p.weights;
  const int kfirst = FORM == kHySplit ? 64 * wave : 0;
  const int kstep = FORM == kHySplit ? 256 : 64;
  v4i acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = (v4i){0, 0, 0, 0};
  if (active) {
    for (int k0 = kfirst; k0 < K; k0 += kstep) {
      const int k = k0 + 16 * q;
      const v4i a = conv_hybrid_frag<VEC>(img, k, K, iy0, ix0, padb, p, dv);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        if (t < nt) {  // wave-uniform
          v4i bw = (v4i){0, 0, 0, 0};
          if (k < KP) bw = *(const v4i*)(wbase + (long)min(n0 + 16 * t + r16, N - 1) * KP + k);
          acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bw, a, acc[t], 0, 0, 0);
        }
      }
    }
  }
  if constexpr (FORM == kHySplit) {
    // integer partial sums: any order of addition gives the rule's sum
    __shared__ v4i part[3][NT][64];
    if (wave > 0) {
#pragma unroll
      for (int t = 0; t < NT; ++t) part[wave - 1][t][lane] = acc[t];
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int w = 0; w < 3; ++w)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const v4i o = part[w][t][lane];
        acc[t].x += o.x; acc[t].y += o.y; acc[t].z += o.z; acc[t].w += o.w;
      }
  }
  const int m = m0 + r16;
  if (!active || m >= M) return;
  const float s = p.in_scale[b];
  const bool vec_out = (N & 3) == 0 && ((uintptr_t)p.output & 15) == 0;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int nb = n0 + 16 * t + 4 * q;
    if (t >= nt || nb >= N) continue;
    float y[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = min(nb + r, N - 1);
      const int32_t dot = (int32_t)((uint32_t)acc[t][r] - (uint32_t)(off * p.w_row_sum[c]));
      const float bias = p.bias ? p.bias[c] : 0.f;
      float v;
      if (p.per_channel) {
        const float t1 = (float)dot * p.w_scale[c];
        const float t2 = t1 * s;
        v = t2 + bias;
      } else {
        const float sc = s * p.w_scale[c];
        const float prod = (float)dot * sc;
        v = bias + prod;
      }
      y[r] = fminf(fmaxf(v, p.act_min), p.act_max);
    }
    float* out = p.output + (long)m * N + nb;
    if (vec_out) {
      *(float4*)out = make_float4(y[0], y[1], y[2], y[3]);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (nb + r < N) out[r] = y[r];
    }
  }
}

// ---- dwconv_hybrid_kernel --------------------------------------------------------------

struct DwHyDivs {
  FastDiv groups, out_w, out_hw, dm;
};

template <bool VEC4>
__global__ __launch_bounds__(256) void dwconv_hybrid_kernel(bh_conv_hybrid_params p, DwHyDivs dv, unsigned total) {
  const unsigned idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= total) return;
  const int m = (int)dv.groups.div(idx);
  const int c0 = 4 * (int)(idx - (unsigned)m * dv.groups.d);
  const int b = (int)dv.out_hw.div((uint32_t)m);
  const int rem = m - b * (int)dv.out_hw.d;
  const int oy = (int)dv.out_w.div((uint32_t)rem);
  const int ox = rem - oy * p.out_w;
  const int iy0 = oy * p.stride_h - p.pad_h, ix0 = ox * p.stride_w - p.pad_w;
  const int8_t* img = p.q + (long)b * p.in_h * p.in_w * p.in_c;
  const int C = p.out_c;
  int ci[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) ci[i] = (int)dv.dm.div((uint32_t)min(c0 + i, C - 1));
  int32_t acc[4] = {0, 0, 0, 0}, wsum[4] = {0, 0, 0, 0};
  for (int ky = 0; ky < p.k_h; ++ky) {
    const int iy = iy0 + ky * p.dil_h;
    if ((unsigned)iy >= (unsigned)p.in_h) continue;
    for (int kx = 0; kx < p.k_w; ++kx) {
      const int ix = ix0 + kx * p.dil_w;
      if ((unsigned)ix >= (unsigned)p.in_w) continue;
      const int8_t* px = img + ((long)iy * p.in_w + ix) * p.in_c;
      const int8_t* wp = p.weights + (long)(ky * p.k_w + kx) * C + c0;
      if constexpr (VEC4) {
        const uint32_t xv = *(const uint32_t*)(px + c0), wv = *(const uint32_t*)wp;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          acc[i] += sbyte(xv, i) * sbyte(wv, i);
          wsum[i] += sbyte(wv, i);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (c0 + i < C) {
            const int32_t w = wp[i];
            acc[i] += (int32_t)px[ci[i]] * w;
            wsum[i] += w;
          }
        }
      }
    }
  }
  const float s = p.in_scale[b];
  const int32_t off = p.in_offset[b];
  float y[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = min(c0 + i, C - 1);
    const int32_t dot = acc[i] - off * wsum[i];
    const float sc = p.w_scale[c] * s;
    const float prod = (float)dot * sc;
    const float v = prod + (p.bias ? p.bias[c] : 0.f);
    y[i] = fminf(fmaxf(v, p.act_min), p.act_max);
  }
  float* out = p.output + (long)m * C + c0;
  if ((C & 3) == 0 && ((uintptr_t)p.output & 15) == 0) {
    *(float4*)out = make_float4(y[0], y[1], y[2], y[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (c0 + i < C) out[i] = y[i];
  }
}

// ---- checks and launchers --------------------------------------------------------------

static int conv_hybrid_refuse(const char* who, const char* why) {
  static thread_local char msg[160];
  snprintf(msg, sizeof(msg), "%s: %s", who, why);
  bh_set_last_error(msg);
  return BH_EINVAL;
}

static int dq_chunks(const bh_dynquant_items_params& p) { return (p.item_size + BH_DYNQUANT_CHUNK - 1) / BH_DYNQUANT_CHUNK; }

static bool dq_one_launch(const bh_dynquant_items_params& p) {
  return p.form == 1 || (p.form == 0 && p.item_size <= BH_DYNQUANT_ONE_LAUNCH_MAX);
}

static const char* dynquant_items_check(const bh_dynquant_items_params* p) {
  if (!p) return "null parameter block";
  if (!p->input || !p->q || !p->scale || !p->offset) return "null pointer";
  if (p->items <= 0 || p->item_size <= 0) return "non-positive extent";
  if (p->form < 0 || p->form > 2) return "form must be 0, 1 or 2";
  if ((long long)p->items * p->item_size > INT32_MAX) return "a tensor of 2^31 or more elements";
  if (((uintptr_t)p->input | (uintptr_t)p->scale | (uintptr_t)p->offset) & 3) return "float / int32 operands must be 4-byte aligned";
  if (!dq_one_launch(*p)) {
    if (!p->pairs) return "null pointer (the two-launch form needs pairs)";
    if ((uintptr_t)p->pairs & 7) return "pairs must be 8-byte aligned";
  }
  return nullptr;
}

// the shape and pointer rules both product launchers share
static const char* conv_hybrid_common(const bh_conv_hybrid_params* p) {
  if (!p) return "null parameter block";
  if (!p->q || !p->in_scale || !p->in_offset || !p->weights || !p->w_scale || !p->output) return "null pointer";
  if (p->batch <= 0 || p->in_h <= 0 || p->in_w <= 0 || p->in_c <= 0 || p->out_h <= 0 || p->out_w <= 0 || p->out_c <= 0 ||
      p->k_h <= 0 || p->k_w <= 0)
    return "non-positive extent";
  if (p->stride_h <= 0 || p->stride_w <= 0 || p->dil_h <= 0 || p->dil_w <= 0) return "non-positive stride or dilation";
  if (p->pad_h < 0 || p->pad_w < 0) return "negative padding";
  if ((long long)p->batch * p->in_h * p->in_w * p->in_c > INT32_MAX ||
      (long long)p->batch * p->out_h * p->out_w * p->out_c > INT32_MAX)
    return "a tensor of 2^31 or more elements";
  // every tap index stays within one row / column of padding arithmetic: no overflow below
  if ((long long)(p->out_h - 1) * p->stride_h + (long long)(p->k_h - 1) * p->dil_h > INT32_MAX / 2 ||
      (long long)(p->out_w - 1) * p->stride_w + (long long)(p->k_w - 1) * p->dil_w > INT32_MAX / 2)
    return "a tensor of 2^31 or more elements";
  if (((uintptr_t)p->in_scale | (uintptr_t)p->in_offset | (uintptr_t)p->w_scale | (uintptr_t)p->bias | (uintptr_t)p->output) & 3)
    return "float / int32 operands must be 4-byte aligned";
  return nullptr;
}

static const char* conv2d_hybrid_check(const bh_conv_hybrid_params* p) {
  if (const char* why = conv_hybrid_common(p)) return why;
  if (!p->w_row_sum) return "null pointer";
  const long long K = (long long)p->k_h * p->k_w * p->in_c;
  if (K > 65535) return "k_h * k_w * in_c > 65,535 (the int32 sum)";
  if (p->k_pad < K || p->k_pad % 16 != 0) return "k_pad must be a multiple of 16 and >= k_h * k_w * in_c";
  if ((long long)p->out_c * p->k_pad > INT32_MAX) return "a tensor of 2^31 or more elements";
  if ((uintptr_t)p->weights & 15) return "packed weights must be 16-byte aligned";
  if ((uintptr_t)p->w_row_sum & 3) return "float / int32 operands must be 4-byte aligned";
  return nullptr;
}

static const char* dwconv2d_hybrid_check(const bh_conv_hybrid_params* p) {
  if (const char* why = conv_hybrid_common(p)) return why;
  if (p->depth_multiplier <= 0 || (long long)p->in_c * p->depth_multiplier != p->out_c)
    return "out_c must be in_c * depth_multiplier";
  if ((long long)p->k_h * p->k_w > 65535) return "k_h * k_w > 65,535 (the int32 sum)";
  if ((long long)p->k_h * p->k_w * p->out_c > INT32_MAX) return "a tensor of 2^31 or more elements";
  return nullptr;
}

template <int FORM, int NT>
static void conv_hybrid_launch(const bh_conv_hybrid_params& p, int vec, hipStream_t s) {
  ConvHyDivs dv;
  dv.out_w = FastDiv(p.out_w);
  dv.out_hw = FastDiv(p.out_h * p.out_w);
  dv.in_c = FastDiv(p.in_c);
  dv.k_w = FastDiv(p.k_w);
  const int M = p.batch * p.out_h * p.out_w;
  const int gn = (p.out_c + 16 * NT - 1) / (16 * NT);
  const int rows = FORM == kHyTiles ? 64 : 16;
  const unsigned grid = (unsigned)((M + rows - 1) / rows) * (unsigned)gn;
  if (vec == 16) BH_LAUNCH((conv_hybrid_kernel<16, FORM, NT>), dim3(grid), dim3(256), 0, s, p, dv, gn);
  else if (vec == 4) BH_LAUNCH((conv_hybrid_kernel<4, FORM, NT>), dim3(grid), dim3(256), 0, s, p, dv, gn);
  else BH_LAUNCH((conv_hybrid_kernel<1, FORM, NT>), dim3(grid), dim3(256), 0, s, p, dv, gn);
}

// Which form a layer takes.  A workgroup's tile is 64 rows x 64 channels (4
// channel tiles per wave, the gathered fragment used four times) when that
// still gives kHyWideGrid workgroups; below that, 64 rows x 16 channels; and
// when even those are fewer than kHyWideGrid and K has more than two 64-byte
// steps, 16 rows x 16 channels with the K-steps dealt to the 4 waves (the
// 14 x 14 and 7 x 7 layers, the classifier head).
constexpr long kHyWideGrid = 256;
static int conv_hybrid_form(const bh_conv_hybrid_params& p) {
  const long M = (long)p.batch * p.out_h * p.out_w, N = p.out_c;
  const long K = (long)p.k_h * p.k_w * p.in_c;
  const long tiles4 = ((M + 63) / 64) * ((N + 63) / 64), tiles1 = ((M + 63) / 64) * ((N + 15) / 16);
  if (tiles4 >= kHyWideGrid) return 4;
  if (K > 128 && tiles1 < kHyWideGrid) return 0;
  return 1;
}

}  // namespace bh

extern "C" int bh_dynquant_items_check(const bh_dynquant_items_params* p) {
  const char* why = bh::dynquant_items_check(p);
  return why ? bh::conv_hybrid_refuse("bh_dynquant_items", why) : 0;
}

extern "C" const char* bh_dynquant_items_kernel(const bh_dynquant_items_params* p) {
  if (bh::dynquant_items_check(p)) return "";
  return bh::dq_one_launch(*p) ? "dynquant_item_kernel" : "dynquant_minmax_kernel+dynquant_items_kernel";
}

extern "C" int bh_dynquant_items(const bh_dynquant_items_params* pp, bh_stream_t stream) {
  using namespace bh;
  if (const char* why = dynquant_items_check(pp)) return conv_hybrid_refuse("bh_dynquant_items", why);
  const bh_dynquant_items_params& p = *pp;
  hipStream_t s = (hipStream_t)stream;
  // float4 loads and dword stores: every item and every chunk starts on their boundary
  const bool vec4 = p.item_size % 4 == 0 && ((uintptr_t)p.input & 15) == 0 && ((uintptr_t)p.q & 3) == 0;
  if (dq_one_launch(p)) {
    if (vec4) BH_LAUNCH((dynquant_item_kernel<true>), dim3(p.items), dim3(kDqBlock), 0, s, p);
    else BH_LAUNCH((dynquant_item_kernel<false>), dim3(p.items), dim3(kDqBlock), 0, s, p);
    return bh_check_launch("dynquant_item_kernel");
  }
  const int chunks = dq_chunks(p);
  const FastDiv cd((uint32_t)chunks);
  const unsigned grid = (unsigned)p.items * (unsigned)chunks;  // <= 2^31 / 4096 workgroups
  if (vec4) BH_LAUNCH((dynquant_minmax_kernel<true>), dim3(grid), dim3(kDqBlock), 0, s, p, cd);
  else BH_LAUNCH((dynquant_minmax_kernel<false>), dim3(grid), dim3(kDqBlock), 0, s, p, cd);
  if (int rc = bh_check_launch("dynquant_minmax_kernel")) return rc;
  if (vec4) BH_LAUNCH((dynquant_items_kernel<true>), dim3(grid), dim3(kDqBlock), 0, s, p, cd);
  else BH_LAUNCH((dynquant_items_kernel<false>), dim3(grid), dim3(kDqBlock), 0, s, p, cd);
  return bh_check_launch("dynquant_items_kernel");
}

extern "C" int bh_conv2d_hybrid_check(const bh_conv_hybrid_params* p) {
  const char* why = bh::conv2d_hybrid_check(p);
  return why ? bh::conv_hybrid_refuse("bh_conv2d_hybrid", why) : 0;
}

extern "C" const char* bh_conv2d_hybrid_kernel(const bh_conv_hybrid_params* p) {
  return bh::conv2d_hybrid_check(p) ? "" : "conv_hybrid_kernel";
}

extern "C" int bh_conv2d_hybrid(const bh_conv_hybrid_params* pp, bh_stream_t stream) {
  using namespace bh;
  if (const char* why = conv2d_hybrid_check(pp)) return conv_hybrid_refuse("bh_conv2d_hybrid", why);
  const bh_conv_hybrid_params& p = *pp;
  const uintptr_t al = (uintptr_t)p.q | (uintptr_t)p.in_c;
  const int vec = al % 16 == 0 ? 16 : (al % 4 == 0 ? 4 : 1);
  const int form = conv_hybrid_form(p);
  if (form == 0) conv_hybrid_launch<kHySplit, 1>(p, vec, (hipStream_t)stream);
  else if (form == 1) conv_hybrid_launch<kHyTiles, 1>(p, vec, (hipStream_t)stream);
  else conv_hybrid_launch<kHyTiles, 4>(p, vec, (hipStream_t)stream);
  return bh_check_launch("conv_hybrid_kernel");
}

extern "C" int bh_dwconv2d_hybrid_check(const bh_conv_hybrid_params* p) {
  const char* why = bh::dwconv2d_hybrid_check(p);
  return why ? bh::conv_hybrid_refuse("bh_dwconv2d_hybrid", why) : 0;
}

extern "C" const char* bh_dwconv2d_hybrid_kernel(const bh_conv_hybrid_params* p) {
  return bh::dwconv2d_hybrid_check(p) ? "" : "dwconv_hybrid_kernel";
}

extern "C" int bh_dwconv2d_hybrid(const bh_conv_hybrid_params* pp, bh_stream_t stream) {
  using namespace bh;
  if (const char* why = dwconv2d_hybrid_check(pp)) return conv_hybrid_refuse("bh_dwconv2d_hybrid", why);
  const bh_conv_hybrid_params& p = *pp;
  DwHyDivs dv;
  const int groups = (p.out_c + 3) / 4;
  dv.groups = FastDiv((uint32_t)groups);
  dv.out_w = FastDiv(p.out_w);
  dv.out_hw = FastDiv(p.out_h * p.out_w);
  dv.dm = FastDiv(p.depth_multiplier);
  const unsigned total = (unsigned)(p.batch * p.out_h * p.out_w) * (unsigned)groups;  // <= output elements < 2^31
  const unsigned grid = (total + 255u) / 256u;
  const bool vec4 = p.depth_multiplier == 1 && p.in_c % 4 == 0 && (((uintptr_t)p.q | (uintptr_t)p.weights) & 3) == 0;
  hipStream_t s = (hipStream_t)stream;
  if (vec4) BH_LAUNCH((dwconv_hybrid_kernel<true>), dim3(grid), dim3(256), 0, s, p, dv, total);
  else BH_LAUNCH((dwconv_hybrid_kernel<false>), dim3(grid), dim3(256), 0, s, p, dv, total);
  return bh_check_launch("dwconv_hybrid_kernel");
}
