// ARG_MAX / ARG_MIN on gfx950 (TFLite arg_min_max.cc ->
// reference_ops::ArgMinMax).  The reference walks the axis sequentially,
// starting at element 0 and replacing the running extreme only on a strict
// comparison, so the FIRST extreme wins, a float NaN is never "greater" (it is
// selected only when it is element 0) and -0.0 == +0.0.  ARG_MIN is ARG_MAX
// of the negated key (exact for int32 keys of 8-bit values and for floats:
// negation flips the order, keeps equality and keeps NaN a NaN), so every
// form below is a first-maximum search.
//
// Two kernels behind bh_argminmax:
//   argminmax_kernel      a thread per output position.  inner == 1: the
//                         thread owns one contiguous row (C = 21 class
//                         scores of a pixel); 8-bit rows are read as the
//                         aligned dwords that cover them (a dword that holds
//                         one valid byte lies inside the tensor's pages), the
//                         bytes outside the row skipped.  inner > 1: the walk
//                         is strided by `inner`, neighbouring threads on
//                         neighbouring positions, so each step is one
//                         coalesced read.
//   argminmax_row_kernel  inner == 1 and axis_len >= 64 (1,001 class logits):
//                         a wave per row; lane l scans elements l, l + 64, ..
//                         and keeps (key, index); a __shfl_xor butterfly then
//                         merges lanes, preferring the smaller index on equal
//                         keys.  NaNs never enter a lane's running pair; a
//                         row whose element 0 is NaN answers 0 as the
//                         sequential loop does.
// No scratch, atomics or host step: both capture into a hipGraph.
#include <limits.h>

#include "common.hpp"

namespace bh {

template <typename K>
struct ArgKey;
template <>
struct ArgKey<int32_t> {
  static __device__ __forceinline__ int32_t lowest() { return INT_MIN; }
};
template <>
struct ArgKey<float> {
  static __device__ __forceinline__ float lowest() { return -__builtin_inff(); }
};

// key of element i of a row of type IN_TYPE (negated for ARG_MIN)
template <int IN_TYPE>
__device__ __forceinline__ auto arg_key(const void* base, long i, bool is_min) {
  if constexpr (IN_TYPE == BH_ARG_F32) {
    const float v = ((const float*)base)[i];
    return is_min ? -v : v;
  } else {
    const int32_t v = IN_TYPE == BH_ARG_I8 ? (int32_t)((const int8_t*)base)[i] : (int32_t)((const uint8_t*)base)[i];
    return is_min ? -v : v;
  }
}

__device__ __forceinline__ void arg_store(void* out, long o, int32_t idx, int out_bytes) {
  if (out_bytes == 8) ((v2i*)out)[o] = (v2i){idx, 0};
  else ((int32_t*)out)[o] = idx;
}

template <int IN_TYPE>
__global__ __launch_bounds__(256) void argminmax_kernel(bh_argminmax_params p, long total) {
  const long o = (long)blockIdx.x * 256 + threadIdx.x;
  if (o >= total) return;
  const bool is_min = p.is_min != 0;
  const int L = (int)p.axis_len;
  int32_t idx = 0;
  if (p.inner == 1 && IN_TYPE != BH_ARG_F32) {
    // contiguous 8-bit row [o * L, o * L + L): the aligned dwords covering it
    const uintptr_t first = (uintptr_t)p.input + (uintptr_t)(o * L);
    const uintptr_t a0 = first & ~(uintptr_t)3;
    const int skip = (int)(first - a0);
    const int words = (skip + L + 3) >> 2;
    int32_t best = 0;
    for (int w = 0; w < words; ++w) {
      const uint32_t d = *(const uint32_t*)(a0 + 4 * (uintptr_t)w);
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int i = 4 * w + b - skip;
        if (i < 0 || i >= L) continue;
        const uint32_t byte = (d >> (8 * b)) & 0xffu;
        int32_t k = IN_TYPE == BH_ARG_I8 ? (int32_t)(int8_t)byte : (int32_t)byte;
        k = is_min ? -k : k;
        if (i == 0 || k > best) {
          best = k;
          idx = i;
        }
      }
    }
  } else {
    const long a = o / p.inner;
    const long base = a * p.axis_len * p.inner + (o - a * p.inner);
    auto best = arg_key<IN_TYPE>(p.input, base, is_min);
    for (int i = 1; i < L; ++i) {
      const auto k = arg_key<IN_TYPE>(p.input, base + (long)i * p.inner, is_min);
      if (k > best) {
        best = k;
        idx = i;
      }
    }
  }
  arg_store(p.output, o, idx, p.out_bytes);
}

template <int IN_TYPE>
__global__ __launch_bounds__(256) void argminmax_row_kernel(bh_argminmax_params p) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.outer) return;  // whole waves leave together: the shuffles below see full waves
  const int lane = threadIdx.x & 63;
  const bool is_min = p.is_min != 0;
  const int L = (int)p.axis_len;
  const long base = row * p.axis_len;
  using K = decltype(arg_key<IN_TYPE>(p.input, 0, false));
  K best = ArgKey<K>::lowest();
  int32_t idx = INT_MAX;
  for (int i = lane; i < L; i += 64) {
    const K k = arg_key<IN_TYPE>(p.input, base + i, is_min);
    if (k > best || (k == best && i < idx)) {
      best = k;
      idx = i;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const K ob = __shfl_xor(best, m, 64);
    const int32_t oi = __shfl_xor(idx, m, 64);
    if (ob > best || (ob == best && oi < idx)) {
      best = ob;
      idx = oi;
    }
  }
  if (lane == 0) {
    if constexpr (IN_TYPE == BH_ARG_F32) {
      const float first = ((const float*)p.input)[base];
      if (first != first) idx = 0;  // element 0 is NaN: nothing is ever greater
    }
    arg_store(p.output, row, idx, p.out_bytes);
  }
}

static bool arg_row_form(const bh_argminmax_params& p) { return p.inner == 1 && p.axis_len >= 64; }

}  // namespace bh

extern "C" const char* bh_argminmax_kernel(const bh_argminmax_params* p) {
  return p && bh::arg_row_form(*p) ? "argminmax_row_kernel" : "argminmax_kernel";
}

extern "C" int bh_argminmax(const bh_argminmax_params* pp, bh_stream_t s) {
  if (!pp || !pp->input || !pp->output || pp->outer <= 0 || pp->axis_len <= 0 || pp->inner <= 0 ||
      pp->in_type < BH_ARG_I8 || pp->in_type > BH_ARG_F32 || (pp->out_bytes != 4 && pp->out_bytes != 8) ||
      ((uintptr_t)pp->output % pp->out_bytes) != 0 || (pp->in_type == BH_ARG_F32 && ((uintptr_t)pp->input % 4) != 0)) {
    bh_set_last_error("bh_argminmax: invalid parameters");
    return BH_EINVAL;
  }
  const bh_argminmax_params& p = *pp;
  const long total = p.outer * p.inner;
  if (p.axis_len >= INT32_MAX || total / p.inner != p.outer || (total + 255) / 256 >= INT32_MAX) {
    bh_set_last_error("bh_argminmax: tensor too large");
    return BH_EINVAL;
  }
  hipStream_t st = (hipStream_t)s;
  if (bh::arg_row_form(p)) {
    const dim3 grid((unsigned)((p.outer + 3) / 4));
    if (p.in_type == BH_ARG_I8) BH_LAUNCH(bh::argminmax_row_kernel<BH_ARG_I8>, grid, dim3(256), 0, st, p);
    else if (p.in_type == BH_ARG_U8) BH_LAUNCH(bh::argminmax_row_kernel<BH_ARG_U8>, grid, dim3(256), 0, st, p);
    else BH_LAUNCH(bh::argminmax_row_kernel<BH_ARG_F32>, grid, dim3(256), 0, st, p);
    return bh_check_launch("argminmax_row_kernel");
  }
  const dim3 grid((unsigned)((total + 255) / 256));
  if (p.in_type == BH_ARG_I8) BH_LAUNCH(bh::argminmax_kernel<BH_ARG_I8>, grid, dim3(256), 0, st, p, total);
  else if (p.in_type == BH_ARG_U8) BH_LAUNCH(bh::argminmax_kernel<BH_ARG_U8>, grid, dim3(256), 0, st, p, total);
  else BH_LAUNCH(bh::argminmax_kernel<BH_ARG_F32>, grid, dim3(256), 0, st, p, total);
  return bh_check_launch("argminmax_kernel");
}
