// BATCH_MATMUL for gfx950: out[b] = lhs[b] x rhs[b], both operands activations
// (nothing is packed at prepare time).  An operand is described by strides
// (bh_batch_matmul_params), so adj_x / adj_y and broadcast batch dims are data:
// an operand is either K-contiguous (its k stride is 1) or K-strided (its row /
// column stride is 1).
//
// bmm_mfma_kernel (int8, v_mfma_i32_16x16x64_i8): a workgroup is 4 waves on
// the 4 adjacent 16-row tiles of one 16-column tile (NT = 1) or of four
// adjacent ones (NT = 4: a wave's lhs fragment feeds four products) of one
// matrix; a K-step is 64 bytes.  As in conv_grouped_mfma_kernel the product is taken transposed
// (D^T = rhs^T x lhs^T: lane (q, r) supplies column n0 + r and row m0 + r at
// k = 16q .. 16q + 15 and ends up with columns n0 + 4q .. + 3 of row m0 + r),
// so a lane's four results are four consecutive output bytes.
//
// Operand loads (bmm_frag.hpp, shared with attention.hip).  A K-contiguous
// operand is read straight from global memory,
// 16 bytes per lane in 16 / 8 / 4 / 1-byte units (the widest that the
// operand's base and its row and batch strides allow); a unit that straddles K
// falls to bytes, and bytes past K are zero.  A K-strided operand is staged
// per K-step: the workgroup's 256 threads read the 64 (k) x 16 NT (columns, rhs)
// or 64 (k) x 64 (rows, lhs) block along its contiguous dimension (dwords when
// base and stride allow, else bytes) and write it TRANSPOSED into LDS, one
// kPitch-byte line per column / row, so that the fragment read is one
// ds_read_b128 of line r at byte 16q.  All 4 waves read the same rhs lines.
// Two other transposed reads are built and pinned by hint (bmm_lds_frag): the
// block staged as it lies (dword LDS writes) and read by 16 byte gathers, or by
// two ds_read_b64_tr_b8.  Measured on the six P V attention rows
// the byte gathers are 0.3 - 0.6 us behind the transposing writes on every
// row; tr_b8 is 0.1 - 0.3 us behind on four rows and level on the two large
// batch-24 ones (0.05 - 0.08 us ahead in one run, behind in another), so the
// first form, which also needs the least LDS, is routed.
//
// Stores.  The transposed accumulator gives a lane 4 consecutive output
// bytes, so stores are dwords (N % 4 == 0 and a 4-byte aligned output) or
// bytes; 16-byte stores would need a cross-lane exchange and are not built.
//
// LDS pitch.  kPitch = 80 = 64 + 16: a ds_read_b128 is served in 16-lane
// groups over 16-byte slots, 16 slots to the 256-byte bank row.  Lane (q, r)
// reads slot 5r + q; for fixed q the map r -> 5r + q mod 16 is a bijection
// (5 is odd), so the 16 lanes of one q hit 16 distinct slots; a pitch of 64
// would put r and r + 4 on one slot (4-way).  The transposing byte writes of
// the staging are NOT conflict-free (threads t and t + 4 write neighbouring
// bytes of one dword) and were not tuned.
//
// Zero points.  With a' = a - z_l, b' = b - z_r:
//   sum a'b' = sum ab - z_r sum_k a[i,k] - z_l sum_k b[k,j] + K z_l z_r.
// Both sums depend on run-time data: a second and third MFMA per K-step
// against a ones fragment give sum_k a (per row, on the lane) and sum_k b
// (per column, in the registers) in the accumulator's own layout.  A sum
// whose multiplier is 0 is skipped (wave-uniform test).  Every term is
// bounded by K 2^14, hence K <= 32767.
//
// bmm_f32_kernel: 16 x 16 outputs per workgroup through two LDS tiles, one
// k-ordered multiply-add chain per output (compiled without contraction).
#include <climits>

#include "bmm_frag.hpp"
#include "common.hpp"
#include "conv_epilogue.hpp"

namespace bh {

// LS / RS: the lhs / rhs is K-strided (staged through LDS); VEC: fragment
// unit of the K-contiguous operands; NT: 16-column tiles per wave (the lhs
// fragment of a K-step feeds NT products); TR: the transposed read of the
// staged operands (bmm_lds_frag)
template <bool LS, bool RS, int VEC, int NT, int TR>
__global__ __launch_bounds__(256) void bmm_mfma_kernel(bh_batch_matmul_params p, int gn, int fast) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[(64 + (TR == 0 ? 16 * NT : 64)) * kBmmPitch];
  uint8_t* ldsA = lds;
  uint8_t* ldsB = lds + 64 * kBmmPitch;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int r16 = lane & 15;
  const int q = lane >> 4;
  // column tiles fastest: neighbouring workgroups read the same lhs rows
  const int bm = (int)blockIdx.x / gn;
  const int bn = (int)blockIdx.x - bm * gn;
  const int b1 = blockIdx.y, b0 = blockIdx.z;
  const int M = p.m, N = p.n, K = p.k;
  const int mblk = bm * 64;
  const int m0 = mblk + wave * 16;
  const int n0 = bn * 16 * NT;
  const bool active = m0 < M;  // whole wave; an idle wave still stages and meets the barriers
  const uint8_t* A = (const uint8_t*)p.lhs + (long)b0 * p.lhs_bstride[0] + (long)b1 * p.lhs_bstride[1];
  const uint8_t* B = (const uint8_t*)p.rhs + (long)b0 * p.rhs_bstride[0] + (long)b1 * p.rhs_bstride[1];
  // this lane's lhs row / rhs columns, clamped: results of the clamped ones are never stored
  const uint8_t* arow = A + (long)min(m0 + r16, M - 1) * p.lhs_row_stride;
  const uint8_t* bcol[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) bcol[t] = B + (long)min(n0 + 16 * t + r16, N - 1) * p.rhs_col_stride;
  const bool need_rs = p.rhs_zp != 0;  // z_r sum_k a[i, k]
  const bool need_cs = p.lhs_zp != 0;  // z_l sum_k b[k, j]
  const v4i ones = (v4i){0x01010101, 0x01010101, 0x01010101, 0x01010101};

  v4i acc[NT], cs[NT], rs = (v4i){0, 0, 0, 0};
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    acc[t] = (v4i){0, 0, 0, 0};
    cs[t] = (v4i){0, 0, 0, 0};
  }
  for (int k0 = 0; k0 < K; k0 += 64) {
    if constexpr (LS || RS) {
      __syncthreads();  // the previous step's fragment reads
      if constexpr (LS && TR == 0) bmm_stage<64>(ldsA, A, p.lhs_k_stride, k0, K, mblk, M);
      if constexpr (LS && TR != 0) bmm_stage_rows<64>(ldsA, A, p.lhs_k_stride, k0, K, mblk, M);
      if constexpr (RS && TR == 0) bmm_stage<16 * NT>(ldsB, B, p.rhs_k_stride, k0, K, n0, N);
      if constexpr (RS && TR != 0) bmm_stage_rows<16 * NT>(ldsB, B, p.rhs_k_stride, k0, K, n0, N);
      __syncthreads();
    }
    if (active) {
      v4i a;
      if constexpr (LS) a = bmm_lds_frag<TR>(ldsA, wave * 16, r16, q);
      else a = bmm_frag<VEC>(arow, k0 + 16 * q, K);
      if (need_rs) rs = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, a, rs, 0, 0, 0);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        if (t > 0 && n0 + 16 * t >= N) break;  // whole workgroup: the tile lies past N
        v4i b;
        if constexpr (RS) b = bmm_lds_frag<TR>(ldsB, 16 * t, r16, q);
        else b = bmm_frag<VEC>(bcol[t], k0 + 16 * q, K);
        acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(b, a, acc[t], 0, 0, 0);
        if (need_cs) cs[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(b, ones, cs[t], 0, 0, 0);
      }
    }
  }

  const int m = m0 + r16;
  if (!active || m >= M) return;
  const int32_t kzz = K * p.lhs_zp * p.rhs_zp;  // the true K
  const ChanQ cq = chan_q(p.mult, p.shift, p.out_zp);
  const bool vec_store = (N & 3) == 0 && ((uintptr_t)p.out & 3) == 0;
  uint8_t* orow = (uint8_t*)p.out + (((long)b0 * p.batch[1] + b1) * M + m) * N;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int nb = n0 + 16 * t + 4 * q;
    if (nb >= N) break;  // later tiles start further right
    uint32_t packed = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int32_t s = acc[t][r] - p.rhs_zp * rs[r] - p.lhs_zp * cs[t][r] + kzz;
      const int32_t v = fast ? requant_out<true>(s, cq, p.out_zp, -128, 127) : requant_out<false>(s, cq, p.out_zp, -128, 127);
      packed |= ((uint32_t)v & 0xffu) << (8 * r);
    }
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

// float32: thread (ty, tx) owns out[16 bm + ty][16 bn + tx]; strides in elements
__global__ __launch_bounds__(256) void bmm_f32_kernel(bh_batch_matmul_params p, int gn) {
  __shared__ float sa[16][17], sb[16][17];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int bm = (int)blockIdx.x / gn;
  const int bn = (int)blockIdx.x - bm * gn;
  const int b1 = blockIdx.y, b0 = blockIdx.z;
  const int M = p.m, N = p.n, K = p.k;
  const float* A = (const float*)p.lhs + (long)b0 * p.lhs_bstride[0] + (long)b1 * p.lhs_bstride[1];
  const float* B = (const float*)p.rhs + (long)b0 * p.rhs_bstride[0] + (long)b1 * p.rhs_bstride[1];
  const int row = bm * 16 + ty, col = bn * 16 + tx;
  float acc = 0.f;
  for (int k0 = 0; k0 < K; k0 += 16) {
    // elements outside the matrices are 0 in both tiles: past K they add 0 x 0
    sa[ty][tx] = row < M && k0 + tx < K ? A[(long)row * p.lhs_row_stride + (long)(k0 + tx) * p.lhs_k_stride] : 0.f;
    sb[ty][tx] = k0 + ty < K && col < N ? B[(long)(k0 + ty) * p.rhs_k_stride + (long)col * p.rhs_col_stride] : 0.f;
    __syncthreads();
    const int kn = min(16, K - k0);
    for (int kk = 0; kk < kn; ++kk) acc += sa[ty][kk] * sb[kk][tx];
    __syncthreads();
  }
  if (row < M && col < N) ((float*)p.out)[(((long)b0 * p.batch[1] + b1) * M + row) * N + col] = acc;
}

// the parameter checks shared by the launchers; nullptr = runnable
static const char* bmm_check(const bh_batch_matmul_params* p, int elem_bytes) {
  if (!p) return "null parameter block";
  if (!p->lhs || !p->rhs || !p->out) return "null operand pointer";
  if (p->m <= 0 || p->n <= 0 || p->k <= 0 || p->batch[0] <= 0 || p->batch[1] <= 0) return "non-positive extent";
  if (p->batch[0] > 65535 || p->batch[1] > 65535) return "a batch dim above 65535 (grid y / z)";
  if (elem_bytes == 1 && p->k > 32767) return "K > 32767 (the folded zero-point form needs 4 K 2^14 < 2^31)";
  if (p->lhs_row_stride < 0 || p->lhs_k_stride < 0 || p->rhs_k_stride < 0 || p->rhs_col_stride < 0 ||
      p->lhs_bstride[0] < 0 || p->lhs_bstride[1] < 0 || p->rhs_bstride[0] < 0 || p->rhs_bstride[1] < 0)
    return "negative stride";
  const bool l1 = p->lhs_k_stride == 1, l2 = p->lhs_row_stride == 1;
  const bool r1 = p->rhs_k_stride == 1, r2 = p->rhs_col_stride == 1;
  if (!(l1 || l2) || (l1 && l2 && p->m != 1 && p->k != 1)) return "lhs needs exactly one unit stride";
  if (!(r1 || r2) || (r1 && r2 && p->n != 1 && p->k != 1)) return "rhs needs exactly one unit stride";
  const long long bt = (long long)p->batch[0] * p->batch[1];
  const long long lspan = (p->batch[0] - 1LL) * p->lhs_bstride[0] + (p->batch[1] - 1LL) * p->lhs_bstride[1] +
                          (p->m - 1LL) * p->lhs_row_stride + (p->k - 1LL) * p->lhs_k_stride;
  const long long rspan = (p->batch[0] - 1LL) * p->rhs_bstride[0] + (p->batch[1] - 1LL) * p->rhs_bstride[1] +
                          (p->k - 1LL) * p->rhs_k_stride + (p->n - 1LL) * p->rhs_col_stride;
  if (bt * p->m * p->n > INT32_MAX || lspan >= INT32_MAX || rspan >= INT32_MAX)
    return "a tensor of 2^31 or more elements";
  const long long tiles = ((p->m + 15LL) / 16) * ((p->n + 15LL) / 16);
  if (tiles > INT32_MAX) return "a tensor of 2^31 or more elements";
  if (elem_bytes == 4 && (((uintptr_t)p->lhs | (uintptr_t)p->rhs | (uintptr_t)p->out) & 3))
    return "float operands must be 4-byte aligned";
  if (elem_bytes == 1 && (p->shift > 30 || p->shift < -31 || p->mult < 0)) return "multiplier / shift out of range";
  return nullptr;
}

static int bmm_refuse(const char* who, const char* why) {
  static thread_local char msg[160];
  snprintf(msg, sizeof(msg), "%s: %s", who, why);
  bh_set_last_error(msg);
  return BH_EINVAL;
}

template <bool LS, bool RS, int NT, int TR>
static void bmm_launch_vec(const bh_batch_matmul_params& p, int vec, int fast, hipStream_t s) {
  const int gn = (p.n + 16 * NT - 1) / (16 * NT);
  const dim3 grid((unsigned)(((p.m + 63) / 64) * gn), (unsigned)p.batch[1], (unsigned)p.batch[0]);
  if (vec == 16) BH_LAUNCH((bmm_mfma_kernel<LS, RS, 16, NT, TR>), grid, dim3(256), 0, s, p, gn, fast);
  else if (vec == 8) BH_LAUNCH((bmm_mfma_kernel<LS, RS, 8, NT, TR>), grid, dim3(256), 0, s, p, gn, fast);
  else if (vec == 4) BH_LAUNCH((bmm_mfma_kernel<LS, RS, 4, NT, TR>), grid, dim3(256), 0, s, p, gn, fast);
  else BH_LAUNCH((bmm_mfma_kernel<LS, RS, 1, NT, TR>), grid, dim3(256), 0, s, p, gn, fast);
}

template <int NT, int TR>
static void bmm_launch_tr(const bh_batch_matmul_params& p, bool ls, bool rs, int vec, int fast, hipStream_t s) {
  if (ls && rs) bmm_launch_vec<true, true, NT, TR>(p, vec, fast, s);
  else if (ls) bmm_launch_vec<true, false, NT, TR>(p, vec, fast, s);
  else bmm_launch_vec<false, true, NT, TR>(p, vec, fast, s);
}

template <int NT>
static void bmm_launch_nt(const bh_batch_matmul_params& p, bool ls, bool rs, int vec, int fast, int tr, hipStream_t s) {
  if (!ls && !rs) bmm_launch_vec<false, false, NT, 0>(p, vec, fast, s);
  else if (tr == 2) bmm_launch_tr<NT, 2>(p, ls, rs, vec, fast, s);
  else if (tr == 1) bmm_launch_tr<NT, 1>(p, ls, rs, vec, fast, s);
  else bmm_launch_tr<NT, 0>(p, ls, rs, vec, fast, s);
}

// The transposed read of a staged operand (bmm_lds_frag): 0 transposing
// writes + ds_read_b128, 1 byte gathers, 2 ds_read_b64_tr_b8.  Form 0 is
// routed: it measured fastest or tied on every P V row (file header, DESIGN
// 3f).  BH_BMM_READ_* pin a form.
static int bmm_read_form(const bh_batch_matmul_params& p) {
  if (p.kernel_hint & BH_BMM_READ_B128) return 0;
  if (p.kernel_hint & BH_BMM_READ_GATHER) return 1;
  if (p.kernel_hint & BH_BMM_READ_TR8) return 2;
  return 0;
}

// Column tiles per wave.  Four reuse each lhs fragment four times and
// quarter the workgroups.  Measured (both forms pinned): with a
// both operands K-contiguous they win once the grid is large - 9.8 against
// 14.7 us at 24,576 16 x 16 tiles, 6.9 / 7.2 at 12,168 - are level at 4,608
// and lose by 0.5 - 1.5 us on the batch-1 grids, where a launch sits near
// the dispatch floor and the longer wave is pure latency; with a staged rhs
// they never win (by 0.2 - 2.8 us; the 64-column staging block is mostly
// padding at head dims 36 - 64), and with a staged lhs they were not timed
// and spill SGPRs, so a launch with a staged operand always takes one tile.
// BH_BMM_NT1 / BH_BMM_NT4 pin the form.
static int bmm_col_tiles(const bh_batch_matmul_params& p, bool staged) {
  if (p.kernel_hint & BH_BMM_NT1) return 1;
  if (p.kernel_hint & BH_BMM_NT4) return 4;
  const long long tiles = ((p.m + 15LL) / 16) * ((p.n + 15LL) / 16) * p.batch[0] * p.batch[1];
  return !staged && p.n > 16 && tiles >= 8192 ? 4 : 1;
}

}  // namespace bh

extern "C" int bh_batch_matmul_check(const bh_batch_matmul_params* p, int elem_bytes) {
  if (elem_bytes != 1 && elem_bytes != 4) return bh::bmm_refuse("bh_batch_matmul_check", "elem_bytes must be 1 or 4");
  const char* why = bh::bmm_check(p, elem_bytes);
  return why ? bh::bmm_refuse(elem_bytes == 1 ? "bh_batch_matmul_i8" : "bh_batch_matmul_f32", why) : 0;
}

extern "C" const char* bh_batch_matmul_i8_kernel(const bh_batch_matmul_params* p) {
  return bh::bmm_check(p, 1) ? "" : "bmm_mfma_kernel";
}

extern "C" int bh_batch_matmul_i8(const bh_batch_matmul_params* pp, bh_stream_t stream) {
  using namespace bh;
  if (const char* why = bmm_check(pp, 1)) return bmm_refuse("bh_batch_matmul_i8", why);
  const bh_batch_matmul_params& p = *pp;
  // an operand with both strides 1 (an extent of 1) reads as K-contiguous
  const bool ls = p.lhs_k_stride != 1, rs = p.rhs_k_stride != 1;
  // widest fragment unit of the K-contiguous operands: their bases and their row and batch strides decide
  uintptr_t al = 0;
  if (!ls) al |= (uintptr_t)p.lhs | (uintptr_t)p.lhs_row_stride | (uintptr_t)p.lhs_bstride[0] | (uintptr_t)p.lhs_bstride[1];
  if (!rs) al |= (uintptr_t)p.rhs | (uintptr_t)p.rhs_col_stride | (uintptr_t)p.rhs_bstride[0] | (uintptr_t)p.rhs_bstride[1];
  int vec = al % 16 == 0 ? 16 : (al % 8 == 0 ? 8 : (al % 4 == 0 ? 4 : 1));
  if (p.kernel_hint & BH_BMM_BYTES) vec = 1;
  // single-step requantisation: 1 asks for it, -1 leaves it to the launcher, 0 forces the two-step form;
  // it is taken only where bh_conv_requant_fast_ok holds
  const int fast = p.requant_fast != 0 && bh_conv_requant_fast_ok(&p.mult, &p.shift, 1, p.k, 0);
  hipStream_t s = (hipStream_t)stream;
  const int tr = bmm_read_form(p);
  if (bmm_col_tiles(p, ls || rs) == 4) bmm_launch_nt<4>(p, ls, rs, vec, fast, tr, s);
  else bmm_launch_nt<1>(p, ls, rs, vec, fast, tr, s);
  return bh_check_launch("bmm_mfma_kernel");
}

extern "C" int bh_batch_matmul_f32(const bh_batch_matmul_params* pp, bh_stream_t stream) {
  using namespace bh;
  if (const char* why = bmm_check(pp, 4)) return bmm_refuse("bh_batch_matmul_f32", why);
  const bh_batch_matmul_params& p = *pp;
  const int gn = (p.n + 15) / 16;
  const dim3 grid((unsigned)(((p.m + 15) / 16) * gn), (unsigned)p.batch[1], (unsigned)p.batch[0]);
  BH_LAUNCH(bmm_f32_kernel, grid, dim3(256), 0, (hipStream_t)stream, p, gn);
  return bh_check_launch("bmm_f32_kernel");
}
