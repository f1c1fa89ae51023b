// The ten float32 ops a converter makes of a LayerNormalization over the last
// axis, as one launch for gfx950, with the row quantisation of the hybrid
// FULLY_CONNECTEDs that read the result folded into its epilogue.
//
// Op by op the ten are a mean_kernel that walks a row in one lane, twice, and
// eight element-wise launches at the dispatch floor, on a tensor of a few
// hundred kilobytes.  Here a wave owns a row and the row stays in registers
// from load to store: lane l holds the four consecutive elements
// 256 j + 4 l .. + 3 of every 256-element step j (16 values per lane, so
// depth <= BH_LAYERNORM_F32_MAX_DEPTH = 1024).  A row whose base is 16-byte
// aligned and whose depth is a multiple of 4 is read as float4 and its
// quantised bytes are stored as dwords; any other row is read and stored
// element by element into and from the same lanes, so the arithmetic - and
// with it the order of the two row sums - never depends on alignment, on the
// number of rows or on the row's place in its workgroup.  The per-row scalars
// (m, v, e, r, and the quantisation's scale / offset) are computed redundantly
// in every lane.  gamma and beta are read from global memory (L2 hits after
// the first workgroup).  No LDS, no barrier, no atomics.
//
// band_hip_kernels.h holds the rule.  Built with -ffp-contract=off
// -fhip-fp32-correctly-rounded-divide-sqrt (Makefile): every operation rounds
// on its own, and the divisions and the square root are correctly rounded.
#include "common.hpp"
#include "dynquant.hpp"

namespace bh {

constexpr int kLnF32Steps = BH_LAYERNORM_F32_MAX_DEPTH / (4 * kWave);  // float4 per lane
// rows (waves) per workgroup: at the 196 rows of an encoder block the launch
// is bound by latency, and fewer rows per workgroup spread it over more CUs
#ifndef BH_LNF32_ROWS_PER_BLOCK
#define BH_LNF32_ROWS_PER_BLOCK 2
#endif
constexpr int kLnF32RowsPerBlock = BH_LNF32_ROWS_PER_BLOCK;

// the rule's row sum, second half: an xor butterfly over offsets 32 .. 1
// (float addition commutes, so every lane ends with the same bits)
__device__ __forceinline__ float wave_sum_f32(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o);
  return v;
}

// elements c .. c + 3 of base[0 .. depth), zeros past the end; vec: c + 3 < depth
// or c >= depth for every c asked for, and base + c is 16-byte aligned
__device__ __forceinline__ float4 ln_ld4(const float* base, int c, int depth, bool vec) {
  if (vec) return c < depth ? *(const float4*)(base + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  float4 v;
  v.x = c < depth ? base[c] : 0.f;
  v.y = c + 1 < depth ? base[c + 1] : 0.f;
  v.z = c + 2 < depth ? base[c + 2] : 0.f;
  v.w = c + 3 < depth ? base[c + 3] : 0.f;
  return v;
}

__global__ __launch_bounds__(kLnF32RowsPerBlock * kWave) void layernorm_f32_kernel(bh_layernorm_f32_params p) {
  const int lane = threadIdx.x & (kWave - 1);
  const long row = (long)blockIdx.x * kLnF32RowsPerBlock + (threadIdx.x >> 6);
  if (row >= p.rows) return;  // wave-uniform; the kernel has no barrier
  const int depth = p.depth;
  const bool quads = (depth & 3) == 0;
  const float* x = p.input + row * depth;
  const bool vec_x = quads && ((uintptr_t)x & 15) == 0;
  const float fc = (float)depth;

  float4 v[kLnF32Steps];
  float acc = 0.f;  // + 0: the zeros of absent elements leave the sum's bits alone
#pragma unroll
  for (int j = 0; j < kLnF32Steps; ++j) {
    v[j] = ln_ld4(x, 256 * j + 4 * lane, depth, vec_x);
    acc = acc + v[j].x;
    acc = acc + v[j].y;
    acc = acc + v[j].z;
    acc = acc + v[j].w;
  }
  const float m = wave_sum_f32(acc) / fc;
  acc = 0.f;
#pragma unroll
  for (int j = 0; j < kLnF32Steps; ++j) {
    const int c = 256 * j + 4 * lane;
    const float tx = v[j].x - m, ty = v[j].y - m, tz = v[j].z - m, tw = v[j].w - m;
    acc = acc + (c < depth ? tx * tx : 0.f);
    acc = acc + (c + 1 < depth ? ty * ty : 0.f);
    acc = acc + (c + 2 < depth ? tz * tz : 0.f);
    acc = acc + (c + 3 < depth ? tw * tw : 0.f);
  }
  const float var = wave_sum_f32(acc) / fc;
  const float e = var + p.eps;
  const float r = 1.0f / sqrtf(e);

  const bool vec_g = quads && ((uintptr_t)p.gamma & 15) == 0;
  const bool vec_b = quads && ((uintptr_t)p.beta & 15) == 0;
  float* y = p.output ? p.output + row * depth : nullptr;
  const bool vec_y = quads && ((uintptr_t)y & 15) == 0;
  float mn = 0.f, mx = 0.f;  // min(0, min y), max(0, max y)
#pragma unroll
  for (int j = 0; j < kLnF32Steps; ++j) {
    const int c = 256 * j + 4 * lane;
    const float4 ga = ln_ld4(p.gamma, c, depth, vec_g);
    const float4 be = ln_ld4(p.beta, c, depth, vec_b);
    auto one = [&](float xi, float gi, float bi, bool in) {
      const float g = r * gi;
      const float a = xi * g;
      const float b = m * g;
      const float cc = bi - b;
      return in ? a + cc : 0.f;  // absent elements: 0, neutral in the min / max below
    };
    v[j].x = one(v[j].x, ga.x, be.x, c < depth);
    v[j].y = one(v[j].y, ga.y, be.y, c + 1 < depth);
    v[j].z = one(v[j].z, ga.z, be.z, c + 2 < depth);
    v[j].w = one(v[j].w, ga.w, be.w, c + 3 < depth);
    mn = fminf(mn, fminf(fminf(v[j].x, v[j].y), fminf(v[j].z, v[j].w)));
    mx = fmaxf(mx, fmaxf(fmaxf(v[j].x, v[j].y), fmaxf(v[j].z, v[j].w)));
    if (y) {
      if (vec_y) {
        if (c < depth) *(float4*)(y + c) = v[j];
      } else {
        if (c < depth) y[c] = v[j].x;
        if (c + 1 < depth) y[c + 1] = v[j].y;
        if (c + 2 < depth) y[c + 2] = v[j].z;
        if (c + 3 < depth) y[c + 3] = v[j].w;
      }
    }
  }
  if (!p.q) return;  // wave-uniform

  // the hybrid row rule on the float32 values just formed (dynquant.hpp)
  mn = wave_min(mn);
  mx = wave_max(mx);
  float s, inv;
  int32_t off;
  dq_derive(mn, mx, p.asymmetric != 0, s, inv, off);
  if (lane == 0) {
    p.scale[row] = s;
    p.offset[row] = off;
  }
  const float foff = (float)off;
  const int32_t lo = p.asymmetric ? -128 : -127;
  int8_t* qrow = p.q + row * depth;
  const bool vec_q = quads && ((uintptr_t)qrow & 3) == 0;
#pragma unroll
  for (int j = 0; j < kLnF32Steps; ++j) {
    const int c = 256 * j + 4 * lane;
    if (vec_q) {
      if (c < depth) *(uint32_t*)(qrow + c) = dq_pack(v[j], inv, foff, lo);
    } else {
      if (c < depth) qrow[c] = (int8_t)dq_one(v[j].x, inv, foff, lo);
      if (c + 1 < depth) qrow[c + 1] = (int8_t)dq_one(v[j].y, inv, foff, lo);
      if (c + 2 < depth) qrow[c + 2] = (int8_t)dq_one(v[j].z, inv, foff, lo);
      if (c + 3 < depth) qrow[c + 3] = (int8_t)dq_one(v[j].w, inv, foff, lo);
    }
  }
}

static const char* layernorm_f32_why(const bh_layernorm_f32_params* p) {
  if (!p) return "null parameter block";
  if (!p->input || !p->gamma || !p->beta) return "null input, gamma or beta";
  if (!p->output && !p->q) return "neither output nor q is set";
  if ((p->q != nullptr) != (p->scale != nullptr) || (p->q != nullptr) != (p->offset != nullptr))
    return "q, scale and offset must be all set or all null";
  if (p->rows < 1 || p->depth < 1) return "non-positive rows or depth";
  if (p->depth > BH_LAYERNORM_F32_MAX_DEPTH) return "depth above 1024 (16 values per lane)";
  if (p->rows >= (1l << 31)) return "2^31 or more rows";
  if (((uintptr_t)p->input | (uintptr_t)p->gamma | (uintptr_t)p->beta | (uintptr_t)p->output | (uintptr_t)p->scale |
       (uintptr_t)p->offset) & 3)
    return "float / int32 operands must be 4-byte aligned";
  return nullptr;
}

}  // namespace bh

extern "C" int bh_layernorm_f32_check(const bh_layernorm_f32_params* p) {
  const char* why = bh::layernorm_f32_why(p);
  if (!why) return 0;
  static thread_local char msg[160];
  snprintf(msg, sizeof(msg), "bh_layernorm_f32: %s", why);
  bh_set_last_error(msg);
  return BH_EINVAL;
}

extern "C" const char* bh_layernorm_f32_kernel(const bh_layernorm_f32_params* p) {
  return bh::layernorm_f32_why(p) ? "" : "layernorm_f32_kernel";
}

extern "C" int bh_layernorm_f32(const bh_layernorm_f32_params* p, bh_stream_t stream) {
  if (bh_layernorm_f32_check(p) != 0) return BH_EINVAL;
  const unsigned blocks = (unsigned)((p->rows + bh::kLnF32RowsPerBlock - 1) / bh::kLnF32RowsPerBlock);
  BH_LAUNCH(bh::layernorm_f32_kernel, dim3(blocks), dim3(bh::kLnF32RowsPerBlock * bh::kWave), 0, (hipStream_t)stream,
            *p);
  return bh_check_launch("layernorm_f32_kernel");
}
