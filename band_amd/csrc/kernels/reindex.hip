// The re-indexing ops on gfx950: TRANSPOSE, STRIDED_SLICE, SLICE, SPLIT,
// SPLIT_V, SPACE_TO_DEPTH and DEPTH_TO_SPACE compute nothing - each output
// element is one input element - so all seven are one thing on the device: a
// dense row-major output whose element (i_0, .., i_{r-1}) is input element
// in_offset + sum_d i_d * in_stride[d] (bh_reindex_params).  The host resolves
// an op to that map (executor_internal.h ReindexArgs); this file moves bytes.
//
// The launcher first canonicalises the map (bh_reindex_canonical): unit dims
// go, and dims d, d + 1 merge when in_stride[d] == in_stride[d + 1] *
// out_dims[d + 1], i.e. when stepping d is stepping d + 1 past its end.  A
// channel split of an NHWC tensor becomes [N*H*W][c] with strides [C][1], an
// NHWC -> NCHW transpose [N][C][H*W] with strides [HWC][1][C].  Three kernels:
//
//   reindex_rows_kernel    innermost stride 1.  Both sides are runs of
//                          out_dims[last] * elem_bytes contiguous bytes; a lane
//                          moves V = 16 / 8 / 4 / 1 bytes, the widest that
//                          divides the run length, both base addresses (the
//                          input's with in_offset applied) and every outer
//                          stride in bytes, so every access is naturally
//                          aligned.  Lanes are numbered over all V-byte units
//                          of the output, so a 16-byte run takes one lane and a
//                          wave covers 64 rows: short runs still fill lanes,
//                          and the stores of a wave are one contiguous span.
//   reindex_tile_kernel    innermost stride != 1 but another dim j has input
//                          stride 1 - a transpose - and both j and last are at
//                          least 64 long.  A workgroup moves a 64 x 64 tile of
//                          (j, last) through LDS: loads walk j (input
//                          contiguous), stores walk last (output contiguous).
//   reindex_gather_kernel  the rest (an innermost ::-1 or ::2, a transpose with
//                          a short edge such as NHWC -> NCHW of 3 or 16
//                          channels): a thread per 4 output bytes - one 4-byte
//                          element, or four 1-byte elements each resolved on
//                          its own, since a group may straddle rows - and one
//                          dword store.
//
// Index math is 32-bit FastDiv (common.hpp), so a map of more than 2^31 - 1
// elements is refused.  No scratch, atomics or host step: all three capture
// into a hipGraph.
//
// A map that carries an index tensor (bh_reindex_params.indices: GATHER, whose
// indices are data on the device) is not resolved here: the launcher hands it
// to bh_gather (gather.hip).
#include <limits.h>

#include "band_hip_gather_shared.h"
#include "common.hpp"

namespace bh {

constexpr int kRxRank = BH_REINDEX_MAX_RANK;
constexpr int kRxTile = 64;

// a canonical map as the kernels take it.  rows / gather: dims = the output's
// dims, stride = input bytes per step.  tile: dims = the workgroup grid (tiles
// along j and last, extents elsewhere), stride / ostride = input / output
// elements per grid step.
struct RxMap {
  int rank;
  uint32_t dims[kRxRank];
  FastDiv div[kRxRank];
  long long stride[kRxRank];
  long long ostride[kRxRank];
  const unsigned char* in;  // in_offset applied
  unsigned char* out;
  uint32_t total;  // threads (rows / gather) with work
  uint32_t elems;  // output elements
};

// input byte offset of row-major position r over dims [0, n)
__device__ __forceinline__ long long rx_offset(const RxMap& m, uint32_t r, int n) {
  long long off = 0;
#pragma unroll
  for (int d = kRxRank - 1; d >= 0; --d) {
    if (d < n) {
      const uint32_t q = m.div[d].div(r);
      off += (long long)(r - q * m.dims[d]) * m.stride[d];
      r = q;
    }
  }
  return off;
}

template <typename V>
__global__ __launch_bounds__(256) void reindex_rows_kernel(RxMap m, FastDiv per_row) {
  const uint32_t u = blockIdx.x * 256u + threadIdx.x;
  if (u >= m.total) return;
  const uint32_t row = per_row.div(u);
  const long long off = rx_offset(m, row, m.rank - 1) + (long long)(u - row * per_row.d) * (long long)sizeof(V);
  *(V*)(m.out + (size_t)u * sizeof(V)) = *(const V*)(m.in + off);
}

// LDS: one 32-bit word per element (1-byte elements too: byte-wide LDS
// accesses of 4 lanes share a dword, and a column read would then be 16
// distinct addresses per bank), row pitch 65 words.  ds_write_b32 /
// ds_read_b32 serve a wave as two groups of 32 lanes, bank = word address mod
// 32.  The staging store tile[l][c] has l wave-uniform and c the lane: 32
// consecutive words, 32 banks.  The transposed read tile[c][j] has word
// address 65 c + j, bank (c + j) mod 32 since 65 = 1 (mod 32): 32 lanes, 32
// banks.  At pitch 64 every lane of the read would sit on bank j mod 32, a
// 32-way conflict.  64 * 65 * 4 = 16,640 bytes of static LDS.
template <typename T>
__global__ __launch_bounds__(256) void reindex_tile_kernel(RxMap m, int jpos, long long s_last, long long o_j,
                                                           uint32_t dj, uint32_t dl) {
  __shared__ uint32_t tile[kRxTile][kRxTile + 1];
  uint32_t r = blockIdx.x;
  long long ioff = 0, ooff = 0;
  uint32_t j0 = 0, l0 = 0;
#pragma unroll
  for (int d = kRxRank - 1; d >= 0; --d) {
    if (d < m.rank) {
      const uint32_t q = m.div[d].div(r);
      const uint32_t i = r - q * m.dims[d];
      ioff += (long long)i * m.stride[d];
      ooff += (long long)i * m.ostride[d];
      if (d == m.rank - 1) l0 = i * kRxTile;
      if (d == jpos) j0 = i * kRxTile;
      r = q;
    }
  }
  const uint32_t c = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const T* in = (const T*)m.in + ioff;
  T* out = (T*)m.out + ooff;
  // edge tiles: a lane outside the tensor neither loads nor stores
#pragma unroll 4
  for (uint32_t l = w; l < kRxTile; l += 4)
    if (j0 + c < dj && l0 + l < dl) tile[l][c] = (uint32_t)in[(long long)c + (long long)l * s_last];
  __syncthreads();
#pragma unroll 4
  for (uint32_t j = w; j < kRxTile; j += 4)
    if (j0 + j < dj && l0 + c < dl) out[(long long)j * o_j + c] = (T)tile[c][j];
}

template <int EB>
__global__ __launch_bounds__(256) void reindex_gather_kernel(RxMap m, int dword_stores) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= m.total) return;
  if constexpr (EB == 4) {
    *(uint32_t*)(m.out + 4 * (size_t)t) = *(const uint32_t*)(m.in + rx_offset(m, t, m.rank));
  } else {
    const uint32_t e0 = 4u * t;
    const uint32_t n = m.elems - e0 < 4u ? m.elems - e0 : 4u;
    uint32_t word = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b)
      if (b < n) word |= (uint32_t)m.in[rx_offset(m, e0 + b, m.rank)] << (8 * b);
    if (n == 4 && dword_stores) {
      *(uint32_t*)(m.out + e0) = word;
    } else {  // the last, partial group, or an output off a dword boundary
      for (uint32_t b = 0; b < n; ++b) m.out[e0 + b] = (unsigned char)(word >> (8 * b));
    }
  }
}

// ---- host --------------------------------------------------------------------
static const char* rx_canonical(const bh_reindex_params& p, bh_reindex_params* c) {
  if (p.indices) return "bh_reindex: a map with indices has no canonical form";
  if (p.rank < 0) return "bh_reindex: invalid parameters";
  if (p.rank > kRxRank) return "bh_reindex: rank > 6";
  if (p.elem_bytes != 1 && p.elem_bytes != 4) return "bh_reindex: elem_bytes must be 1 or 4";
  *c = bh_reindex_params{};
  c->elem_bytes = p.elem_bytes;
  c->in_offset = p.in_offset;
  c->input = p.input;
  c->output = p.output;
  long long total = 1;
  int n = 0;
  for (int d = 0; d < p.rank; ++d) {
    if (p.out_dims[d] <= 0) return "bh_reindex: invalid parameters";
    total *= p.out_dims[d];
    if (total > INT_MAX) return "bh_reindex: more than 2^31 - 1 elements";
    if (p.out_dims[d] == 1) continue;
    if (n > 0 && c->in_stride[n - 1] == p.in_stride[d] * p.out_dims[d]) {
      c->out_dims[n - 1] *= p.out_dims[d];
      c->in_stride[n - 1] = p.in_stride[d];
    } else {
      c->out_dims[n] = p.out_dims[d];
      c->in_stride[n] = p.in_stride[d];
      ++n;
    }
  }
  if (n == 0) {
    c->out_dims[0] = 1;
    c->in_stride[0] = 1;
    n = 1;
  }
  c->rank = n;
  return nullptr;
}

enum RxPath { kRxRows, kRxTilePath, kRxGather };
static RxPath rx_path(const bh_reindex_params& c, int* jpos) {
  const int last = c.rank - 1;
  if (c.in_stride[last] == 1) return kRxRows;
  // a tile pays only when both of its edges fill a wave: measured on the
  // MI355X (tools/reindex_profile.py) it is 1.2 x (1024^2) to 3.7 x (4096^2
  // bytes, 32 x 112 x 112 x 64) faster than the gather there, but with a
  // 16-channel edge it ties or loses (7.0 / 7.2 us at 32 x 64 x 64 x 16) and
  // with a 3- or 2-wide edge it loses 3 - 7 x (most of each 64 x 64 tile is
  // predicated off), so those go to the gather, whose strided reads hit in L2
  for (int d = last - 1; d >= 0; --d)
    if (c.in_stride[d] == 1 && c.out_dims[d] >= kRxTile && c.out_dims[last] >= kRxTile) {
      *jpos = d;
      return kRxTilePath;
    }
  return kRxGather;
}

static long long rx_elems(const bh_reindex_params& c) {
  long long n = 1;
  for (int d = 0; d < c.rank; ++d) n *= c.out_dims[d];
  return n;
}

// bytes per lane of the rows form
static int rx_rows_width(const bh_reindex_params& c) {
  const long long eb = c.elem_bytes;
  uintptr_t bits = (uintptr_t)(c.out_dims[c.rank - 1] * eb) | ((uintptr_t)c.input + (uintptr_t)(c.in_offset * eb)) |
                   (uintptr_t)c.output;
  for (int d = 0; d + 1 < c.rank; ++d) bits |= (uintptr_t)(c.in_stride[d] * eb);
  return bits % 16 == 0 ? 16 : (bits % 8 == 0 ? 8 : (bits % 4 == 0 ? 4 : 1));
}

}  // namespace bh

extern "C" int bh_reindex_canonical(const bh_reindex_params* p, bh_reindex_params* canonical) {
  const char* err = p && canonical ? bh::rx_canonical(*p, canonical) : "bh_reindex: invalid parameters";
  if (err) {
    bh_set_last_error(err);
    return BH_EINVAL;
  }
  return 0;
}

extern "C" const char* bh_reindex_kernel(const bh_reindex_params* p) {
  if (p && p->indices) {  // GATHER as a map: gather.hip's kernel
    bh_gather_params g;
    return bh_reindex_as_gather(p, &g) ? "" : bh_gather_kernel(&g);
  }
  bh_reindex_params c;
  if (!p || bh::rx_canonical(*p, &c)) return "";
  int jpos = -1;
  switch (bh::rx_path(c, &jpos)) {
    case bh::kRxRows: return "reindex_rows_kernel";
    case bh::kRxTilePath: return "reindex_tile_kernel";
    default: return "reindex_gather_kernel";
  }
}

extern "C" int bh_reindex(const bh_reindex_params* pp, bh_stream_t s) { return bh_reindex_as(pp, 0, s); }

extern "C" int bh_reindex_as(const bh_reindex_params* pp, int gather, bh_stream_t s) {
  using namespace bh;
  if (pp && pp->indices && !gather) {
    bh_gather_params g;
    if (const char* e = bh_reindex_as_gather(pp, &g)) {
      bh_set_last_error(e);
      return BH_EINVAL;
    }
    return bh_gather(&g, s);
  }
  bh_reindex_params c;
  const char* err = pp ? rx_canonical(*pp, &c) : "bh_reindex: invalid parameters";
  if (!err && (!c.input || !c.output || (uintptr_t)c.input % c.elem_bytes || (uintptr_t)c.output % c.elem_bytes))
    err = "bh_reindex: input and output must be non-null and aligned to elem_bytes";
  if (err) {
    bh_set_last_error(err);
    return BH_EINVAL;
  }
  hipStream_t st = (hipStream_t)s;
  const int eb = c.elem_bytes, last = c.rank - 1;
  const long long elems = rx_elems(c);  // <= INT_MAX (rx_canonical)
  RxMap m{};
  m.rank = c.rank;
  m.in = (const unsigned char*)c.input + c.in_offset * eb;
  m.out = (unsigned char*)c.output;
  m.elems = (uint32_t)elems;
  int jpos = -1;
  const RxPath path = gather ? kRxGather : rx_path(c, &jpos);
  if (path == kRxTilePath) {
    long long ost[kRxRank], blocks = 1;
    ost[last] = 1;
    for (int d = last - 1; d >= 0; --d) ost[d] = ost[d + 1] * c.out_dims[d + 1];
    for (int d = 0; d < c.rank; ++d) {
      const bool tiled = d == jpos || d == last;
      m.dims[d] = (uint32_t)(tiled ? (c.out_dims[d] + kRxTile - 1) / kRxTile : c.out_dims[d]);
      m.div[d] = FastDiv(m.dims[d]);
      m.stride[d] = tiled ? kRxTile * c.in_stride[d] : c.in_stride[d];
      m.ostride[d] = tiled ? kRxTile * ost[d] : ost[d];
      blocks *= m.dims[d];  // <= elems
    }
    m.total = (uint32_t)blocks;
    const dim3 grid((unsigned)blocks);
    const uint32_t dj = (uint32_t)c.out_dims[jpos], dl = (uint32_t)c.out_dims[last];
    if (eb == 1)
      BH_LAUNCH(reindex_tile_kernel<uint8_t>, grid, dim3(256), 0, st, m, jpos, c.in_stride[last], ost[jpos], dj, dl);
    else
      BH_LAUNCH(reindex_tile_kernel<uint32_t>, grid, dim3(256), 0, st, m, jpos, c.in_stride[last], ost[jpos], dj, dl);
    return bh_check_launch("reindex_tile_kernel");
  }
  for (int d = 0; d < c.rank; ++d) {
    m.dims[d] = (uint32_t)c.out_dims[d];
    m.div[d] = FastDiv(m.dims[d]);
    m.stride[d] = c.in_stride[d] * eb;
  }
  if (path == kRxRows) {
    const int v = rx_rows_width(c);
    const uint32_t per_row = (uint32_t)((long long)c.out_dims[last] * eb / v);
    m.total = (uint32_t)(elems / c.out_dims[last] * per_row);  // <= elems: v >= eb
    const dim3 grid((m.total + 255u) / 256u);
    const FastDiv pr(per_row);
    if (v == 16) BH_LAUNCH(reindex_rows_kernel<v4i>, grid, dim3(256), 0, st, m, pr);
    else if (v == 8) BH_LAUNCH(reindex_rows_kernel<v2i>, grid, dim3(256), 0, st, m, pr);
    else if (v == 4) BH_LAUNCH(reindex_rows_kernel<uint32_t>, grid, dim3(256), 0, st, m, pr);
    else BH_LAUNCH(reindex_rows_kernel<uint8_t>, grid, dim3(256), 0, st, m, pr);
    return bh_check_launch("reindex_rows_kernel");
  }
  m.total = (uint32_t)(eb == 4 ? elems : (elems + 3) / 4);
  const dim3 grid((m.total + 255u) / 256u);
  if (eb == 4) BH_LAUNCH(reindex_gather_kernel<4>, grid, dim3(256), 0, st, m, 1);
  else BH_LAUNCH(reindex_gather_kernel<1>, grid, dim3(256), 0, st, m, (uintptr_t)c.output % 4 == 0 ? 1 : 0);
  return bh_check_launch("reindex_gather_kernel");
}
