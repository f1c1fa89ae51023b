// Dynamic-range ("hybrid") FULLY_CONNECTED for gfx950: float32 activations,
// constant int8 weights with one scale, each input row quantised to int8 at
// run time, an int8 product, a float32 epilogue.  Restated from memory of
// TFLite's fully_connected.cc EvalHybrid and
// tensor_utils::{Symmetric,Asymmetric}QuantizeFloats; DESIGN 4 holds the rule
// and says what is pinned.  Two launches:
//
// dynquant_rows_kernel: one wave per row, 4 rows per workgroup.  A first pass
// takes the row's min and max (a __shfl_xor butterfly over the lanes), lane 0
// turns them into (scale, 1 / scale, offset) - the asymmetric form in float64 -
// and a __shfl broadcasts the three; a second pass quantises.  Rows of up to
// kDqRegs * 256 floats stay in registers between the passes (float4 per lane
// when the row is 16-byte aligned), longer or unaligned rows are read twice.
//
// fc_hybrid_kernel: [rows x depth] . [units x depth]^T on
// v_mfma_i32_16x16x64_i8, both operands K-contiguous and read straight from
// global memory - the unstaged form of bmm_mfma_kernel, with bmm_frag's
// zero-filled K tail for the quantised rows; the weights are packed with K
// padded to 16 by zeros, so their fragments are whole 16-byte loads.  The
// product is taken transposed (lane (q, r) ends up with units n0 + 4q .. + 3
// of row m0 + r), so a lane's four results are 16 consecutive output bytes.
// A workgroup is 4 waves, and what the four do is the FORM:
//   kRows   rows > 16: the 4 adjacent 16-row tiles of one 16-unit tile.
//   kUnits  rows <= 16, depth <= 128: 4 adjacent 16-unit tiles of the one
//           row tile.
//   kSplit  rows <= 16, depth > 128 (the classifier head): one 16-unit tile,
//           wave w takes the K-steps w, w + 4, ...; the partial accumulators
//           meet in LDS and are added as int32, so the sum is the rule's.
// Epilogue, per element, every operation rounded on its own (the file is
// built with -ffp-contract=off and the correctly rounded division):
//   dot = acc - offset[row] * w_row_sum[unit]      (int32, exact: depth <= 65,535)
//   y = bias[unit] + (float)dot * (scale[row] * w_scale), clamped.
// No atomics, no scratch.
#include <climits>

#include "bmm_frag.hpp"
#include "common.hpp"
#include "dynquant.hpp"

namespace bh {

constexpr int kDqRowsPerBlock = 4;
constexpr int kDqRegs = 4;  // float4 per lane kept between the passes: rows of up to 1024 floats

template <bool VEC4>
__global__ __launch_bounds__(kDqRowsPerBlock * kWave) void dynquant_rows_kernel(bh_dynquant_params p) {
  const int lane = threadIdx.x & (kWave - 1);
  const long row = (long)blockIdx.x * kDqRowsPerBlock + (threadIdx.x >> 6);
  if (row >= p.rows) return;  // wave-uniform; the kernel has no barrier
  const int depth = p.depth;
  const float* x = p.input + row * depth;
  int8_t* qrow = p.q + row * depth;
  float mn = 0.f, mx = 0.f;  // min(0, min x), max(0, max x); the symmetric r is max(-mn, mx)
  float4 keep[kDqRegs];
  const int nv = depth >> 2;  // VEC4: depth % 4 == 0
  if constexpr (VEC4) {
#pragma unroll
    for (int j = 0; j < kDqRegs; ++j) {
      const int i = lane + kWave * j;
      keep[j] = i < nv ? ((const float4*)x)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      mn = fminf(mn, fminf(fminf(keep[j].x, keep[j].y), fminf(keep[j].z, keep[j].w)));
      mx = fmaxf(mx, fmaxf(fmaxf(keep[j].x, keep[j].y), fmaxf(keep[j].z, keep[j].w)));
    }
    for (int i = lane + kWave * kDqRegs; i < nv; i += kWave) {
      const float4 v = ((const float4*)x)[i];
      mn = fminf(mn, fminf(fminf(v.x, v.y), fminf(v.z, v.w)));
      mx = fmaxf(mx, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
    }
  } else {
    for (int i = lane; i < depth; i += kWave) {
      mn = fminf(mn, x[i]);
      mx = fmaxf(mx, x[i]);
    }
  }
  mn = wave_min(mn);
  mx = wave_max(mx);

  float s = 1.f, inv = 0.f;  // inv 0: every q is the offset, 0
  int32_t off = 0;
  if (lane == 0) dq_derive(mn, mx, p.asymmetric != 0, s, inv, off);  // dynquant.hpp
  s = __shfl(s, 0);
  inv = __shfl(inv, 0);
  off = __shfl(off, 0);
  if (lane == 0) {
    p.scale[row] = s;
    p.offset[row] = off;
  }
  const float foff = (float)off;
  const int32_t lo = p.asymmetric ? -128 : -127;
  if constexpr (VEC4) {
    uint32_t* qw = (uint32_t*)qrow;  // depth % 4 == 0 and an aligned q: dword stores
    auto pack = [&](const float4& v) {
      return ((uint32_t)dq_one(v.x, inv, foff, lo) & 0xffu) | (((uint32_t)dq_one(v.y, inv, foff, lo) & 0xffu) << 8) |
             (((uint32_t)dq_one(v.z, inv, foff, lo) & 0xffu) << 16) | (((uint32_t)dq_one(v.w, inv, foff, lo) & 0xffu) << 24);
    };
#pragma unroll
    for (int j = 0; j < kDqRegs; ++j) {
      const int i = lane + kWave * j;
      if (i < nv) qw[i] = pack(keep[j]);
    }
    for (int i = lane + kWave * kDqRegs; i < nv; i += kWave) qw[i] = pack(((const float4*)x)[i]);
  } else {
    for (int i = lane; i < depth; i += kWave) qrow[i] = (int8_t)dq_one(x[i], inv, foff, lo);
  }
}

enum FcHybridForm { kRows = 0, kUnits = 1, kSplit = 2 };

// VEC: fragment unit of the quantised rows (their base and depth decide)
template <int VEC, int FORM>
__global__ __launch_bounds__(256) void fc_hybrid_kernel(bh_fc_hybrid_params p, int gn) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int r16 = lane & 15;
  const int q = lane >> 4;
  const int M = p.rows, N = p.units, K = p.depth, KP = p.depth_pad;
  int m0, n0;
  if constexpr (FORM == kRows) {
    // unit tiles fastest: neighbouring workgroups read the same quantised rows
    const int bm = (int)blockIdx.x / gn;
    n0 = ((int)blockIdx.x - bm * gn) * 16;
    m0 = bm * 64 + wave * 16;
  } else if constexpr (FORM == kUnits) {
    m0 = 0;
    n0 = (int)blockIdx.x * 64 + wave * 16;
  } else {
    m0 = 0;
    n0 = (int)blockIdx.x * 16;
  }
  const bool active = m0 < M && n0 < N;  // whole wave
  // this lane's row and unit, clamped: results of the clamped ones are never stored
  const uint8_t* arow = (const uint8_t*)p.q + (long)min(m0 + r16, M - 1) * K;
  const uint8_t* brow = (const uint8_t*)p.weights + (long)min(n0 + r16, N - 1) * KP;
  const int kfirst = FORM == kSplit ? 64 * wave : 0;
  const int kstep = FORM == kSplit ? 256 : 64;
  v4i acc = (v4i){0, 0, 0, 0};
  if (active) {
    for (int k0 = kfirst; k0 < K; k0 += kstep) {
      const int k = k0 + 16 * q;
      const v4i a = bmm_frag<VEC>(arow, k, K);
      v4i b = (v4i){0, 0, 0, 0};
      if (k < KP) b = *(const v4i*)(brow + k);  // KP % 16 == 0, bytes past depth are zero
      acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(b, a, acc, 0, 0, 0);
    }
  }
  if constexpr (FORM == kSplit) {
    // integer partial sums: any order of addition gives the rule's dot
    __shared__ v4i part[3][64];
    if (wave > 0) part[wave - 1][lane] = acc;
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int w = 0; w < 3; ++w) {
      const v4i o = part[w][lane];
      acc.x += o.x; acc.y += o.y; acc.z += o.z; acc.w += o.w;
    }
  }
  const int m = m0 + r16;
  const int nb = n0 + 4 * q;
  if (!active || m >= M || nb >= N) return;
  const float sc = p.in_scale[m] * p.w_scale;
  const int32_t off = p.in_offset[m];
  float y[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int u = min(nb + r, N - 1);
    const int32_t dot = (int32_t)((uint32_t)acc[r] - (uint32_t)(off * p.w_row_sum[u]));
    const float prod = (float)dot * sc;
    const float v = (p.bias ? p.bias[u] : 0.f) + prod;
    y[r] = fminf(fmaxf(v, p.act_min), p.act_max);
  }
  float* out = p.output + (long)m * N + nb;
  if ((N & 3) == 0 && ((uintptr_t)p.output & 15) == 0) {
    *(float4*)out = make_float4(y[0], y[1], y[2], y[3]);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (nb + r < N) out[r] = y[r];
  }
}

static int hybrid_refuse(const char* who, const char* why) {
  static thread_local char msg[160];
  snprintf(msg, sizeof(msg), "%s: %s", who, why);
  bh_set_last_error(msg);
  return BH_EINVAL;
}

static const char* dynquant_check(const bh_dynquant_params* p) {
  if (!p) return "null parameter block";
  if (!p->input || !p->q || !p->scale || !p->offset) return "null pointer";
  if (p->rows <= 0 || p->depth <= 0) return "non-positive extent";
  if (p->rows * (long long)p->depth > INT32_MAX) return "a tensor of 2^31 or more elements";
  if (((uintptr_t)p->input | (uintptr_t)p->scale | (uintptr_t)p->offset) & 3) return "float / int32 operands must be 4-byte aligned";
  return nullptr;
}

static const char* fc_hybrid_check(const bh_fc_hybrid_params* p) {
  if (!p) return "null parameter block";
  if (!p->q || !p->in_scale || !p->in_offset || !p->weights || !p->w_row_sum || !p->output) return "null pointer";
  if (p->rows <= 0 || p->depth <= 0 || p->units <= 0) return "non-positive extent";
  if (p->depth > 65535) return "depth > 65,535 (the int32 dot)";
  if (p->depth_pad < p->depth || p->depth_pad % 16 != 0) return "depth_pad must be a multiple of 16 and >= depth";
  if ((long long)p->rows * p->depth > INT32_MAX || (long long)p->rows * p->units > INT32_MAX ||
      (long long)p->units * p->depth_pad > INT32_MAX)
    return "a tensor of 2^31 or more elements";
  if ((uintptr_t)p->weights & 15) return "packed weights must be 16-byte aligned";
  if (((uintptr_t)p->in_scale | (uintptr_t)p->in_offset | (uintptr_t)p->w_row_sum | (uintptr_t)p->bias |
       (uintptr_t)p->output) & 3)
    return "float / int32 operands must be 4-byte aligned";
  return nullptr;
}

template <int FORM>
static void fc_hybrid_launch(const bh_fc_hybrid_params& p, int vec, hipStream_t s) {
  const int gn = (p.units + 15) / 16;
  const unsigned grid = FORM == kRows ? (unsigned)(((p.rows + 63) / 64) * gn)
                                      : (FORM == kUnits ? (unsigned)((p.units + 63) / 64) : (unsigned)gn);
  if (vec == 16) BH_LAUNCH((fc_hybrid_kernel<16, FORM>), dim3(grid), dim3(256), 0, s, p, gn);
  else if (vec == 4) BH_LAUNCH((fc_hybrid_kernel<4, FORM>), dim3(grid), dim3(256), 0, s, p, gn);
  else BH_LAUNCH((fc_hybrid_kernel<1, FORM>), dim3(grid), dim3(256), 0, s, p, gn);
}

}  // namespace bh

extern "C" int bh_dynquant_rows_check(const bh_dynquant_params* p) {
  const char* why = bh::dynquant_check(p);
  return why ? bh::hybrid_refuse("bh_dynquant_rows", why) : 0;
}

extern "C" const char* bh_dynquant_rows_kernel(const bh_dynquant_params* p) {
  return bh::dynquant_check(p) ? "" : "dynquant_rows_kernel";
}

extern "C" int bh_dynquant_rows(const bh_dynquant_params* pp, bh_stream_t stream) {
  using namespace bh;
  if (const char* why = dynquant_check(pp)) return hybrid_refuse("bh_dynquant_rows", why);
  const bh_dynquant_params& p = *pp;
  const unsigned blocks = (unsigned)((p.rows + kDqRowsPerBlock - 1) / kDqRowsPerBlock);
  // float4 loads and dword stores: every row starts on their boundary
  const bool vec4 = p.depth % 4 == 0 && ((uintptr_t)p.input & 15) == 0 && ((uintptr_t)p.q & 3) == 0;
  if (vec4) BH_LAUNCH((dynquant_rows_kernel<true>), dim3(blocks), dim3(kDqRowsPerBlock * kWave), 0, (hipStream_t)stream, p);
  else BH_LAUNCH((dynquant_rows_kernel<false>), dim3(blocks), dim3(kDqRowsPerBlock * kWave), 0, (hipStream_t)stream, p);
  return bh_check_launch("dynquant_rows_kernel");
}

extern "C" int bh_fc_hybrid_check(const bh_fc_hybrid_params* p) {
  const char* why = bh::fc_hybrid_check(p);
  return why ? bh::hybrid_refuse("bh_fc_hybrid", why) : 0;
}

extern "C" const char* bh_fc_hybrid_kernel(const bh_fc_hybrid_params* p) {
  return bh::fc_hybrid_check(p) ? "" : "fc_hybrid_kernel";
}

extern "C" int bh_fc_hybrid(const bh_fc_hybrid_params* pp, bh_stream_t stream) {
  using namespace bh;
  if (const char* why = fc_hybrid_check(pp)) return hybrid_refuse("bh_fc_hybrid", why);
  const bh_fc_hybrid_params& p = *pp;
  const uintptr_t al = (uintptr_t)p.q | (uintptr_t)p.depth;
  const int vec = al % 16 == 0 ? 16 : (al % 4 == 0 ? 4 : 1);
  hipStream_t s = (hipStream_t)stream;
  if (p.rows > 16) fc_hybrid_launch<kRows>(p, vec, s);
  else if (p.depth <= 128) fc_hybrid_launch<kUnits>(p, vec, s);
  else fc_hybrid_launch<kSplit>(p, vec, s);
  return bh_check_launch("fc_hybrid_kernel");
}
