// GATHER on gfx950: params viewed as [outer][axis_size][inner], a flat list of
// n_idx indices, output [outer][n_idx][inner] = np.take(params, indices, axis).
// The indices are data on the device (an embedding lookup's token ids are a
// model input), so unlike the re-indexing ops (reindex.hip) the map cannot be
// resolved on the host: each output row reads its index first.
//
// One kernel, gather_rows_kernel, in the shape of reindex_rows_kernel: lanes
// are numbered over all V-byte units of the output, V = 16 / 8 / 4 / 1 the
// widest that divides the row length inner * elem_bytes and both base
// addresses, so every access is naturally aligned, a wave's stores are one
// contiguous span whatever the row length (a 16-byte row takes one lane, a
// 768-byte row 48) and short rows still fill lanes.  Per unit: row = u /
// units_per_row and (o, j) = divmod(row, n_idx) by FastDiv, the index load
// (the lanes of a row load one address; the cache serves it once), then the
// source ((o * axis_size + idx) * inner) * elem_bytes + within in 64-bit
// arithmetic.  bh_gather_row (band_hip_gather_shared.h, shared with CpuGather)
// range-checks the index in its own width; a unit whose index is outside
// [0, axis_size) issues no load and stores zeros.
//
// Index math is 32-bit FastDiv over output units, so more than 2^31 - 1 output
// bytes are refused.  No scratch, atomics or host step: the launch captures
// into a hipGraph.
#include <limits.h>

#include "band_hip_gather_shared.h"
#include "common.hpp"

namespace bh {

struct GatherMap {
  const unsigned char* params;
  const void* indices;
  unsigned char* out;
  uint32_t total;       // V-byte units of the output
  int32_t axis_size;
  int32_t index_bytes;  // 4 or 8
  long long row_bytes;  // inner * elem_bytes
};

template <typename V>
__global__ __launch_bounds__(256) void gather_rows_kernel(GatherMap m, FastDiv per_row, FastDiv n_idx) {
  const uint32_t u = blockIdx.x * 256u + threadIdx.x;
  if (u >= m.total) return;
  const uint32_t row = per_row.div(u);
  const uint32_t o = n_idx.div(row);
  const long long idx = bh_gather_row(m.indices, m.index_bytes, (long long)(row - o * n_idx.d), m.axis_size);
  V v = {};
  if (idx >= 0) {
    const long long within = (long long)(u - row * per_row.d) * (long long)sizeof(V);
    v = *(const V*)(m.params + ((long long)o * m.axis_size + idx) * m.row_bytes + within);
  }
  *(V*)(m.out + (size_t)u * sizeof(V)) = v;
}

// ---- host --------------------------------------------------------------------
// bytes per lane
static int gather_width(const bh_gather_params& p) {
  const uintptr_t bits = (uintptr_t)(p.inner * p.elem_bytes) | (uintptr_t)p.params | (uintptr_t)p.output;
  return bits % 16 == 0 ? 16 : (bits % 8 == 0 ? 8 : (bits % 4 == 0 ? 4 : 1));
}

}  // namespace bh

extern "C" int bh_gather_check(const bh_gather_params* p) {
  if (const char* err = bh_gather_refusal(p)) {
    bh_set_last_error(err);
    return BH_EINVAL;
  }
  return 0;
}

extern "C" const char* bh_gather_kernel(const bh_gather_params* p) {
  return bh_gather_refusal(p) ? "" : "gather_rows_kernel";
}

extern "C" int bh_gather(const bh_gather_params* pp, bh_stream_t s) {
  using namespace bh;
  if (bh_gather_check(pp) != 0) return BH_EINVAL;
  const bh_gather_params& p = *pp;
  hipStream_t st = (hipStream_t)s;
  GatherMap m{};
  m.params = (const unsigned char*)p.params;
  m.indices = p.indices;
  m.out = (unsigned char*)p.output;
  m.axis_size = (int32_t)p.axis_size;
  m.index_bytes = p.index_bytes;
  m.row_bytes = (long long)p.inner * p.elem_bytes;
  const int v = gather_width(p);
  const uint32_t per_row = (uint32_t)(m.row_bytes / v);
  m.total = (uint32_t)(p.outer * p.n_idx) * per_row;  // <= output bytes <= INT_MAX (bh_gather_refusal)
  const dim3 grid((m.total + 255u) / 256u);
  const FastDiv pr(per_row), ni((uint32_t)p.n_idx);
  if (v == 16) BH_LAUNCH(gather_rows_kernel<v4i>, grid, dim3(256), 0, st, m, pr, ni);
  else if (v == 8) BH_LAUNCH(gather_rows_kernel<v2i>, grid, dim3(256), 0, st, m, pr, ni);
  else if (v == 4) BH_LAUNCH(gather_rows_kernel<uint32_t>, grid, dim3(256), 0, st, m, pr, ni);
  else BH_LAUNCH(gather_rows_kernel<uint8_t>, grid, dim3(256), 0, st, m, pr, ni);
  return bh_check_launch("gather_rows_kernel");
}
