// The ops a converted int8 LayerNormalization is made of, for gfx950:
// MEAN over the last axis and SQUARED_DIFFERENCE (RSQRT is a bh_lut_u8 table,
// ADD / SUB / MUL are eltwise_pool.hip's).
//
// MEAN over the last axis of a [rows][depth] tensor of a few tens of kilobytes
// is bound by latency, not by bytes: mean_kernel's one thread per output would
// walk a whole row serially in one lane.  mean_rows_kernel gives a row to a
// wave: 64 lanes read it as dwords (after a byte head up to the row's 4-byte
// boundary, before a byte tail), each lane sums its bytes in int32 and a
// __shfl_xor butterfly adds the lanes.  Integer sums are order-free, so the
// result is the reference's.  Rows longer than 64 dwords loop.
//
// Built with -ffp-contract=off (Makefile): QuantizedMeanOrSum's float32
// mean * scale + bias must round twice.
#include "eltwise_ops.hpp"

namespace bh {

constexpr int kMeanRowsPerBlock = 4;

__global__ __launch_bounds__(kMeanRowsPerBlock * kWave) void mean_rows_kernel(bh_mean_rows_params p) {
  const int lane = threadIdx.x & (kWave - 1);
  const long row = (long)blockIdx.x * kMeanRowsPerBlock + (threadIdx.x >> 6);
  if (row >= p.rows) return;  // wave-uniform; the kernel has no barrier
  const bool sgn = p.type == 1;
  const uint8_t* x = (const uint8_t*)p.input + row * p.depth;
  const int head = min((int)((4 - ((uintptr_t)x & 3)) & 3), p.depth);
  const int nd = (p.depth - head) >> 2;
  const int tail = p.depth - head - 4 * nd;
  int32_t acc = 0;
  if (lane < head) acc += ld8(x, lane, sgn);
  const uint32_t* w = (const uint32_t*)(x + head);
  for (int i = lane; i < nd; i += kWave) acc += sum4(w[i], sgn);
  if (lane < tail) acc += ld8(x, head + 4 * nd + lane, sgn);
  acc = wave_sum(acc);
  if (lane == 0)
    ((uint8_t*)p.output)[row] = (uint8_t)mean_rows_finish(acc, p.depth, p.exact, p.scale, p.bias, p.out_zp, sgn);
}

// output-shape divisors for the broadcast index math (FastDiv, host-built)
struct SqdiffDivs {
  FastDiv d3, d2, d1;
};

__global__ __launch_bounds__(256) void eltwise_sqdiff_kernel(bh_eltwise_params p, int n, SqdiffDivs dv) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int t = dv.d3.div(i);
  const int i3 = i - t * (int)dv.d3.d;
  const int t2 = dv.d2.div(t);
  const int i2 = t - t2 * (int)dv.d2.d;
  const int i0 = dv.d1.div(t2);
  const int i1 = t2 - i0 * (int)dv.d1.d;
  const int32_t qa = ld8((const uint8_t*)p.a, bcast_index(p.shape_a, i0, i1, i2, i3), true);
  const int32_t qb = ld8((const uint8_t*)p.b, bcast_index(p.shape_b, i0, i1, i2, i3), true);
  ((uint8_t*)p.out)[i] = (uint8_t)sqdiff_op(p, qa, qb);
}

// ---- the ten ops of a LayerNorm in one launch ------------------------------------
// Op by op they are ten dispatches at the launch floor on a tensor of a few
// tens of kilobytes.  Here a wave owns a row: lane l holds elements l, l + 64,
// ... (16 at most) in registers, the two row sums are butterflies, and the
// per-row scalars (m, v, e, r) are computed redundantly in every lane.  The
// arithmetic is sqdiff_op / elt_op / mean_rows_finish of the single-op kernels
// on the same int8 values, so the stored bytes are the same.
constexpr int kLnPerLane = BH_LAYERNORM_MAX_DEPTH / kWave;
constexpr int kLnRowsPerBlock = 4;

__global__ __launch_bounds__(kLnRowsPerBlock * kWave) void layernorm_i8_kernel(bh_layernorm_params p) {
  __shared__ uint8_t s_table[256];
  __shared__ int8_t s_gamma[BH_LAYERNORM_MAX_DEPTH];
  __shared__ int8_t s_beta[BH_LAYERNORM_MAX_DEPTH];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) s_table[i] = ((const uint8_t*)p.rsqrt_table)[i];
  for (int i = threadIdx.x; i < p.depth; i += blockDim.x) {
    s_gamma[i] = ((const int8_t*)p.gamma)[i];
    s_beta[i] = ((const int8_t*)p.beta)[i];
  }
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1);
  const long row = (long)blockIdx.x * kLnRowsPerBlock + (threadIdx.x >> 6);
  if (row >= p.rows) return;  // after the only barrier
  const int8_t* x = (const int8_t*)p.input + row * p.depth;
  int32_t xv[kLnPerLane];
  int32_t acc = 0;
#pragma unroll
  for (int k = 0; k < kLnPerLane; ++k) {
    const int c = lane + k * kWave;
    xv[k] = c < p.depth ? (int32_t)x[c] : 0;
    acc += xv[k];
  }
  const int32_t m = mean_rows_finish(wave_sum(acc), p.depth, p.mean_x.exact, p.mean_x.scale, p.mean_x.bias,
                                     p.mean_x.out_zp, true);
  acc = 0;
#pragma unroll
  for (int k = 0; k < kLnPerLane; ++k)
    if (lane + k * kWave < p.depth) acc += sqdiff_op(p.sqdiff, xv[k], m);
  const int32_t v = mean_rows_finish(wave_sum(acc), p.depth, p.mean_d.exact, p.mean_d.scale, p.mean_d.bias,
                                     p.mean_d.out_zp, true);
  const int32_t e = elt_op(p.add_eps, v, p.eps_q);
  const int32_t r = (int32_t)(int8_t)s_table[(uint8_t)e];
  int8_t* y = (int8_t*)p.output + row * p.depth;
#pragma unroll
  for (int k = 0; k < kLnPerLane; ++k) {
    const int c = lane + k * kWave;
    if (c < p.depth) {
      const int32_t g = elt_op(p.mul_gamma, r, (int32_t)s_gamma[c]);
      const int32_t a = elt_op(p.mul_x, xv[k], g);
      const int32_t b = elt_op(p.mul_m, m, g);
      const int32_t cc = elt_op(p.sub_beta, (int32_t)s_beta[c], b);
      y[c] = (int8_t)elt_op(p.add_out, a, cc);
    }
  }
}

}  // namespace bh

extern "C" int bh_layernorm_i8_check(const bh_layernorm_params* p) {
  const char* why = nullptr;
  auto add_like = [](const bh_eltwise_params& q) {
    return q.kind == BH_ELT_ADD && q.in_signed && q.left_shift >= 0 && q.left_shift <= 20 && q.a_shift <= 0 &&
           q.b_shift <= 0 && q.o_shift <= 0 && q.a_shift >= -31 && q.b_shift >= -31 && q.o_shift >= -31;
  };
  auto mul_like = [](const bh_eltwise_params& q) {
    return q.kind == BH_ELT_MUL && q.in_signed && q.o_shift <= 31 && q.o_shift >= -31;
  };
  if (!p || !p->input || !p->output || !p->gamma || !p->beta || !p->rsqrt_table) why = "bh_layernorm_i8: null pointer";
  else if (p->rows < 1 || p->depth < 1) why = "bh_layernorm_i8: non-positive rows or depth";
  else if (p->depth > BH_LAYERNORM_MAX_DEPTH) why = "bh_layernorm_i8: depth above 1024 (16 values per lane)";
  else if (p->rows >= (1l << 31)) why = "bh_layernorm_i8: 2^31 or more rows";
  else if (p->mean_x.type != 1 || p->mean_d.type != 1 || p->mean_x.depth != p->depth || p->mean_d.depth != p->depth)
    why = "bh_layernorm_i8: the MEAN blocks must be int8 and of the row's depth";
  else if (p->sqdiff.kind != BH_ELT_SQDIFF || !p->sqdiff.in_signed || p->sqdiff.left_shift != 7 ||
           p->sqdiff.a_shift > 0 || p->sqdiff.b_shift > 0 || p->sqdiff.o_shift > 0 || p->sqdiff.a_shift < -31 ||
           p->sqdiff.b_shift < -31 || p->sqdiff.o_shift < -31)
    why = "bh_layernorm_i8: the SQUARED_DIFFERENCE block is not an int8 BH_ELT_SQDIFF";
  else if (!add_like(p->add_eps) || !add_like(p->sub_beta) || !add_like(p->add_out))
    why = "bh_layernorm_i8: an ADD / SUB block is not an int8 BH_ELT_ADD";
  else if (!mul_like(p->mul_gamma) || !mul_like(p->mul_x) || !mul_like(p->mul_m))
    why = "bh_layernorm_i8: a MUL block is not an int8 BH_ELT_MUL";
  else if (p->eps_q < -128 || p->eps_q > 127) why = "bh_layernorm_i8: eps_q is not an int8 value";
  if (!why) return 0;
  bh_set_last_error(why);
  return BH_EINVAL;
}

extern "C" const char* bh_layernorm_i8_kernel(const bh_layernorm_params* p) {
  return bh_layernorm_i8_check(p) == 0 ? "layernorm_i8_kernel" : "";
}

extern "C" int bh_layernorm_i8(const bh_layernorm_params* p, bh_stream_t stream) {
  if (bh_layernorm_i8_check(p) != 0) return BH_EINVAL;
  const unsigned blocks = (unsigned)((p->rows + bh::kLnRowsPerBlock - 1) / bh::kLnRowsPerBlock);
  BH_LAUNCH(bh::layernorm_i8_kernel, dim3(blocks), dim3(bh::kLnRowsPerBlock * bh::kWave), 0, (hipStream_t)stream, *p);
  return bh_check_launch("layernorm_i8_kernel");
}

extern "C" int bh_mean_rows_check(const bh_mean_rows_params* p) {
  const char* why = nullptr;
  if (!p || !p->input || !p->output) why = "bh_mean_rows: null pointer";
  else if (p->rows < 1 || p->depth < 1) why = "bh_mean_rows: non-positive rows or depth";
  else if (p->type != 1 && p->type != 2) why = "bh_mean_rows: type must be 1 (int8) or 2 (uint8)";
  else if ((long)p->depth * 255 >= (1l << 31)) why = "bh_mean_rows: depth * 255 >= 2^31 (the int32 row sum)";
  else if (p->rows >= (1l << 31)) why = "bh_mean_rows: 2^31 or more rows";
  if (!why) return 0;
  bh_set_last_error(why);
  return BH_EINVAL;
}

extern "C" const char* bh_mean_rows_kernel(const bh_mean_rows_params* p) {
  return bh_mean_rows_check(p) == 0 ? "mean_rows_kernel" : "";
}

extern "C" int bh_mean_rows(const bh_mean_rows_params* p, bh_stream_t stream) {
  if (bh_mean_rows_check(p) != 0) return BH_EINVAL;
  const unsigned blocks = (unsigned)((p->rows + bh::kMeanRowsPerBlock - 1) / bh::kMeanRowsPerBlock);
  BH_LAUNCH(bh::mean_rows_kernel, dim3(blocks), dim3(bh::kMeanRowsPerBlock * bh::kWave), 0, (hipStream_t)stream, *p);
  return bh_check_launch("mean_rows_kernel");
}

int bh_eltwise_sqdiff_i8(const bh_eltwise_params* pp, bh_stream_t stream) {
  if (!pp || !pp->a || !pp->b || !pp->out) {
    bh_set_last_error("bh_eltwise_i8: null pointer (SQUARED_DIFFERENCE)");
    return BH_EINVAL;
  }
  const bh_eltwise_params& p = *pp;
  if (!p.in_signed) {
    bh_set_last_error("bh_eltwise_i8: SQUARED_DIFFERENCE is int8 only");
    return BH_EINVAL;
  }
  if (p.left_shift < 0 || p.left_shift > 7 || p.a_shift > 0 || p.b_shift > 0 || p.o_shift > 0 || p.a_shift < -31 ||
      p.b_shift < -31 || p.o_shift < -31) {
    bh_set_last_error("bh_eltwise_i8: SQUARED_DIFFERENCE shifts out of range");
    return BH_EINVAL;
  }
  long n = 1;
  for (int d = 0; d < 4; ++d) {
    if (p.shape_o[d] <= 0 || (p.shape_a[d] != p.shape_o[d] && p.shape_a[d] != 1) ||
        (p.shape_b[d] != p.shape_o[d] && p.shape_b[d] != 1)) {
      bh_set_last_error("bh_eltwise_i8: bad shape (SQUARED_DIFFERENCE)");
      return BH_EINVAL;
    }
    n *= p.shape_o[d];
  }
  if (n >= INT32_MAX) {
    bh_set_last_error("bh_eltwise_i8: tensor too large for 32-bit indexing");
    return BH_EINVAL;
  }
  bh::SqdiffDivs dv;
  dv.d3 = bh::FastDiv(p.shape_o[3]);
  dv.d2 = bh::FastDiv(p.shape_o[2]);
  dv.d1 = bh::FastDiv(p.shape_o[1]);
  BH_LAUNCH(bh::eltwise_sqdiff_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, (int)n,
            dv);
  return bh_check_launch("eltwise_sqdiff_kernel");
}
