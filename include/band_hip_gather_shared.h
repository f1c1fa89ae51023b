/* What gather_rows_kernel's launcher (kernels/gather.hip) and its host twin
 * CpuGather (backend/hip/cpu_kernels.cc) share as inline code, so that both
 * workers refuse the same parameters and treat an index outside
 * [0, axis_size) alike. */
#ifndef BAND_HIP_GATHER_SHARED_H_
#define BAND_HIP_GATHER_SHARED_H_

#include <limits.h>
#include <stdint.h>

#include "band_hip_kernels.h"

#if defined(__HIPCC__)
#define BH_HOST_DEVICE __host__ __device__
#else
#define BH_HOST_DEVICE
#endif

/* Index j of `indices` (index_bytes 4: int32, 8: int64), compared in its own
 * width before anything is narrowed - an int64 index is never truncated first
 * - or -1 when it lies outside [0, axis_size). */
static inline BH_HOST_DEVICE int64_t bh_gather_row(const void* indices, int index_bytes, int64_t j,
                                                   int32_t axis_size) {
  if (index_bytes == 8) {
    const int64_t v = ((const int64_t*)indices)[j];
    return v >= 0 && v < (int64_t)axis_size ? v : -1;
  }
  const int32_t v = ((const int32_t*)indices)[j];
  return v >= 0 && v < axis_size ? (int64_t)v : -1;
}

/* What bh_gather refuses, as the message bh_last_error gives, or null; pure host. */
static inline const char* bh_gather_refusal(const bh_gather_params* p) {
  if (!p) return "bh_gather: invalid parameters";
  if (!p->params || !p->indices || !p->output) return "bh_gather: params, indices and output must be non-null";
  if (p->elem_bytes != 1 && p->elem_bytes != 4) return "bh_gather: elem_bytes must be 1 or 4";
  if (p->index_bytes != 4 && p->index_bytes != 8) return "bh_gather: index_bytes must be 4 or 8";
  if (p->outer < 1 || p->axis_size < 1 || p->n_idx < 1 || p->inner < 1) return "bh_gather: invalid parameters";
  if ((uintptr_t)p->params % p->elem_bytes || (uintptr_t)p->output % p->elem_bytes)
    return "bh_gather: params and output must be aligned to elem_bytes";
  if ((uintptr_t)p->indices % p->index_bytes) return "bh_gather: indices must be aligned to index_bytes";
  /* each factor first: the products then stay far inside 64 bits */
  if (p->outer > INT_MAX || p->axis_size > INT_MAX || p->n_idx > INT_MAX || p->inner > INT_MAX ||
      p->outer * p->n_idx > INT_MAX || p->outer * p->n_idx * p->inner > INT_MAX / p->elem_bytes)
    return "bh_gather: more than 2^31 - 1 output bytes";
  return 0;
}

/* The bh_gather_params of a map with indices (bh_reindex_params.indices), or
 * the message bh_last_error gives for a map that is not of that form; pure host. */
static inline const char* bh_reindex_as_gather(const bh_reindex_params* p, bh_gather_params* g) {
  if (!p || !g || !p->indices || p->rank != 3 || p->in_offset != 0 || p->index_range < 1 || p->out_dims[2] < 1 ||
      p->in_stride[2] != 1 || p->in_stride[1] != p->out_dims[2] ||
      p->in_stride[0] != p->index_range * (int64_t)p->out_dims[2])
    return "bh_reindex: a map with indices must be [outer][n_idx][inner] over [outer][index_range][inner]";
  g->elem_bytes = p->elem_bytes;
  g->index_bytes = p->index_bytes;
  g->outer = p->out_dims[0];
  g->axis_size = p->index_range;
  g->n_idx = p->out_dims[1];
  g->inner = p->out_dims[2];
  g->params = p->input;
  g->indices = p->indices;
  g->output = p->output;
  return bh_gather_refusal(g);
}

#endif  /* BAND_HIP_GATHER_SHARED_H_ */
