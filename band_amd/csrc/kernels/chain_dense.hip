// Dense (throughput) form of the fused pointwise chain for gfx950:
//   DEPTHWISE_CONV_2D 3x3 -> CONV_2D 1x1 [-> ADD residual] [-> CONV_2D 1x1]
// the same TFLite 2.9.2 kernels chain_kernel (fused_chain.hip) stands in for,
// bit-identical to it.
//
// For chains whose grid gives every CU several 64-pixel workgroups (the
// 112x112 and 56x56 layers at batch 24 / 32: 6 - 25 workgroups per CU), where
// a launch's time is resident waves x progress per wave and not one
// workgroup's latency.  The form is shaped for residency:
//   * a wave owns its 16 pixels through all three phases and keeps them in a
//     slab of LDS no other wave touches, so after the residual tables are
//     built there is NO workgroup barrier: the four waves of a workgroup
//     drift apart and cover each other's load rounds, as do the 6 - 8 waves
//     a SIMD holds;
//   * one item per load round (one depthwise channel group, one 1x1 channel
//     tile), the next 1x1 tile's filter fragments and constants prefetched
//     behind the current tile's MFMAs - a one-deep pipeline instead of the
//     issue-everything-early rounds of the latency forms;
//   * the first 1x1's output is staged once (the second 1x1's operand rows)
//     and stored to HBM from there, no second staging tile;
//   * compiled for WPE waves per SIMD (__launch_bounds__'s second argument),
//     no scratch (profiles/r12a_kernel_resources.txt).
// Layout of a wave's slab: [16][S1] depthwise output, reused as [16][N2] for
// the second 1x1's output; [16][S2] the first 1x1's output.
#include <algorithm>
#include <climits>

#include "chain_dw.hpp"
#include "common.hpp"
#include "residual_add.hpp"

namespace bh {

struct DenseLds {
  int S1, S2, slab, off_pl, off_add;
  size_t bytes;
};

static DenseLds dense_lds(const bh_chain_params& p) {
  DenseLds L;
  // rows of k_pad + 32 bytes, as chain_lds: a ds_read_b128 lane group's 16
  // rows land on 16 distinct bank slots
  L.S1 = p.pw1.k_pad + 32;
  L.S2 = (p.has_pw2 ? p.pw2.k_pad : (p.pw1.out_c + 15) / 16 * 16) + 32;
  const int dl_row = std::max(L.S1, p.has_pw2 ? (p.pw2.out_c + 15) / 16 * 16 : 0);
  L.off_pl = 16 * dl_row;
  L.slab = L.off_pl + 16 * L.S2;
  L.off_add = 4 * L.slab;
  L.bytes = (size_t)L.off_add + (p.pw1.residual ? 512 * sizeof(int) : 0);
  return L;
}

// this wave's `rows` staged pixels (row stride `stride`, N bytes each, N % 4
// == 0) to their contiguous run of HBM
__device__ __forceinline__ void dense_copy_rows(const unsigned char* src, int stride, uint8_t* dst, int N, int rows,
                                                int lane) {
  const bool v16 = (N & 15) == 0;
  const int u = v16 ? N >> 4 : N >> 2;  // units per pixel
  const float rcp = 1.0f / (float)u;
  for (int i = lane; i < rows * u; i += 64) {
    const int r = (int)(((float)i + 0.5f) * rcp);
    const int k = i - r * u;
    if (v16) *(v4i*)(dst + (long)r * N + k * 16) = *(const v4i*)(src + r * stride + k * 16);
    else *(uint32_t*)(dst + (long)r * N + k * 4) = *(const uint32_t*)(src + r * stride + k * 4);
  }
}

// what one lane needs of channel tile t of a 1x1 layer: KX K-steps' filter
// fragments of its channel row and the channel's folded bias, multiplier,
// shift.  All four arrays are read through buffer resources: the lane's part
// of an address (its row of a tile, its K offset) is computed once, the tile
// and K-step move in the scalar offset, so a round costs no vector address
// arithmetic; a channel past out_c reads 0 (range-checked) and is not kept.
struct DenseConv {
  __amdgpu_buffer_rsrc_t w, be, mu, sh;
  int wv, cv;  // this lane's byte offsets into a tile's filter rows / constants
  int tile_w;  // bytes of one tile's filter rows
};
__device__ __forceinline__ DenseConv dense_conv(const bh_conv_params& c, int r16, int g) {
  DenseConv d;
  d.w = __builtin_amdgcn_make_buffer_rsrc((void*)c.weights, (short)0, c.n_pad * c.k_pad, 0x00020000);
  d.be = __builtin_amdgcn_make_buffer_rsrc((void*)c.bias_eff, (short)0, c.out_c * 4, 0x00020000);
  d.mu = __builtin_amdgcn_make_buffer_rsrc((void*)c.mult, (short)0, c.out_c * 4, 0x00020000);
  d.sh = __builtin_amdgcn_make_buffer_rsrc((void*)c.shift, (short)0, c.out_c * 4, 0x00020000);
  d.wv = r16 * c.k_pad + g * 16;
  d.cv = r16 * 4;
  d.tile_w = 16 * c.k_pad;
  return d;
}
template <int KX>
struct DenseTile {
  v4i w[KX];
  int be, mu, sh;
};
template <int KX>
__device__ __forceinline__ void dense_filter_load(const DenseConv& c, int t, int k0, int KS, v4i (&w)[KX]) {
  typedef unsigned int v4u __attribute__((ext_vector_type(4)));
#pragma unroll
  for (int u = 0; u < KX; ++u) {
    if (k0 + u < KS) {
      const v4u v = __builtin_amdgcn_raw_buffer_load_b128(c.w, c.wv, t * c.tile_w + (k0 + u) * 64, 0);
      w[u] = (v4i){(int)v.x, (int)v.y, (int)v.z, (int)v.w};
    } else {
      w[u] = (v4i){0, 0, 0, 0};
    }
  }
}
template <int KX>
__device__ __forceinline__ void dense_tile_load(const DenseConv& c, int t, int k0, int KS, DenseTile<KX>& d) {
  dense_filter_load<KX>(c, t, k0, KS, d.w);
  d.be = (int)__builtin_amdgcn_raw_buffer_load_b32(c.be, c.cv, t * 64, 0);
  d.mu = (int)__builtin_amdgcn_raw_buffer_load_b32(c.mu, c.cv, t * 64, 0);
  d.sh = (int)__builtin_amdgcn_raw_buffer_load_b32(c.sh, c.cv, t * 64, 0);
}

// Phase A of the dense form: chain_dw_mfma's arithmetic (chain_dw.hpp: the
// block-diagonal MFMA tile, the column borrow by ds_bpermute) for a wave that
// owns its block, one channel group per load round.  INTERIOR: every tap of
// every pixel of the block lies inside the image (wave-uniform, most blocks of
// a 112- or 56-wide layer), so the loaded dwords are the operands and the
// twelve zero-point selects per group are not issued.
template <bool FAST, bool INTERIOR>
__device__ __forceinline__ void dense_dw_groups(const bh_dwconv_params& d, const __amdgpu_buffer_rsrc_t rsrc,
                                                const int (&off)[3], const bool (&ok)[3], bool need, int src4, int r16,
                                                int g, unsigned char* dl, int S1) {
  typedef unsigned int v4u __attribute__((ext_vector_type(4)));
  const int zfill = (int)splat_byte(d.in_zp);
  const int dsel = r16 >> 2;
  const int bsh = 8 * (r16 & 3);
  // this lane's filter byte of K-step s in the tap table row (bh_pack_dw_taps)
  const int tsel1 = g == 0 ? 0 : 1, tbit1 = g == 0 ? 24 : 8 * (g - 1);
  const int tbit2 = g < 2 ? 8 * (2 + g) : bsh;
  const int G = d.out_c >> 4;
  for (int cg = 0; cg < G; ++cg) {
    const int c0 = cg * 16;
    // a lane that does not load (a borrowing lane, group 3) never uses what it
    // holds here - bpermute or a select replaces it, or it meets zero filter
    // bytes - so its registers are left as they are instead of being zeroed
    v4u v[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) asm volatile("" : "=v"(v[s].x), "=v"(v[s].y), "=v"(v[s].z), "=v"(v[s].w));
    if (need) {
#pragma unroll
      for (int s = 0; s < 3; ++s) v[s] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off[s] + c0, 0, 0);
    }
    const int c = c0 + r16;  // this lane's result channel
    const v4i tw = *(const v4i*)(d.taps + 4 * c);
    const int32_t mu = d.mult[c], sh = d.shift[c];
    v4i xf[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      if (INTERIOR) xf[s] = (v4i){(int)v[s].x, (int)v[s].y, (int)v[s].z, (int)v[s].w};
      else xf[s] = (v4i){ok[s] ? (int)v[s].x : zfill, ok[s] ? (int)v[s].y : zfill, ok[s] ? (int)v[s].z : zfill,
                         ok[s] ? (int)v[s].w : zfill};
#pragma unroll
      for (int j = 0; j < 4; ++j) xf[s][j] = __builtin_amdgcn_ds_bpermute(src4, xf[s][j]);
    }
    const uint32_t t0 = (uint32_t)tw.x, t1 = (uint32_t)tw.y, t2 = (uint32_t)tw.z;
    uint32_t wb[3];
    wb[0] = (t0 >> (8 * g)) & 0xffu;
    wb[1] = ((tsel1 ? t1 : t0) >> tbit1) & 0xffu;
    wb[2] = ((g < 2 ? t1 : t2) >> tbit2) & 0xffu;
    v4i acc = (v4i){tw.w, tw.w, tw.w, tw.w};
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const int w = g < 3 ? (int)(wb[s] << bsh) : 0;
      const v4i wf = (v4i){dsel == 0 ? w : 0, dsel == 1 ? w : 0, dsel == 2 ? w : 0, dsel == 3 ? w : 0};
      acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(xf[s], wf, acc, 0, 0, 0);
    }
    const ChanQ q = chan_q(mu, sh, d.out_zp);
    int32_t o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = requant_out<FAST>(acc[r], q, d.out_zp, d.act_min, d.act_max);
    stage4(dl, S1, 4 * g, c, o);
  }
}

template <bool FAST>
__device__ __forceinline__ void dense_dw(const bh_dwconv_params& d, const ChainDivs& dv, int m, bool mval, int lane,
                                         int r16, int g, unsigned char* dl, int S1) {
  const int C = d.out_c;
  const int mm = mval ? m : 0;
  const int t = dv.out_w.div(mm);
  const int ox = mm - t * d.out_w;
  const int n = dv.out_h.div(t);
  const int oy = t - n * d.out_h;
  const int iy = oy * d.stride_h, ix = ox * d.stride_w, row0 = n * d.in_h;
  // lane group g takes filter column g (group 3 idles); a lane whose column
  // is another lane's of the same block and output row borrows its dwords
  const int gx = g * d.dil_w;
  const int dd = (g == 1 || g == 2) && gx % d.stride_w == 0 ? gx / d.stride_w : 0;
  const bool borrow = dd > 0 && r16 + dd < 16 && ox + dd < d.out_w;
  const bool need = g < 3 && !borrow;
  const int src4 = (borrow ? r16 + dd : lane) << 2;
  int off[3];
  bool ok[3];
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int y = iy + s * d.dil_h - d.pad_h, x = ix + gx - d.pad_w;
    ok[s] = mval && g < 3 && y >= 0 && y < d.in_h && x >= 0 && x < d.in_w;
    off[s] = ok[s] ? ((row0 + y) * d.in_w + x) * C : 0;
  }
  const __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)d.input, (short)0, d.batch * d.in_h * d.in_w * C, 0x00020000);
  // group 3's operand bytes meet zero filter bytes, so only groups 0 - 2 count
  const bool interior = __builtin_amdgcn_ballot_w64(g < 3 && !(ok[0] && ok[1] && ok[2])) == 0;
  if (interior) dense_dw_groups<FAST, true>(d, rsrc, off, ok, need, src4, r16, g, dl, S1);
  else dense_dw_groups<FAST, false>(d, rsrc, off, ok, need, src4, r16, g, dl, S1);
}

// orders this wave's LDS writes before its later LDS reads (the slab is the
// wave's own: no other wave's accesses are involved)
__device__ __forceinline__ void dense_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// KX: K-steps of the second 1x1 held in registers (K <= 64 * KX)
template <bool FAST, int KX, int WPE>
__global__ __launch_bounds__(256, WPE) void chain_dense_kernel(bh_chain_params cp, int P, DenseLds L, ChainDivs dv) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63;
  const int pb = threadIdx.x >> 6;  // this wave's pixel block
  const int r16 = lane & 15;
  const int g = lane >> 4;
  const int mw = xcd_block(blockIdx.x, gridDim.x) * 64 + pb * 16;  // the wave's first pixel
  unsigned char* dl = smem + pb * L.slab;  // [16][S1], later [16][N2]
  unsigned char* pl = dl + L.off_pl;       // [16][S2]
  // residual ADD: both operands' rescalings as 256-entry tables (chain_kernel)
  const int* add_tab = (const int*)(smem + L.off_add);
  if (cp.pw1.residual) {
    residual_tab_build((int*)(smem + L.off_add), cp.pw1, threadIdx.x, 256);
    __syncthreads();  // the only workgroup barrier
  }
  if (mw >= P) return;  // an empty block of the last workgroup
  const int rows = min(16, P - mw);
  const int orow = 4 * g;  // first of this lane's 4 result rows in the slab

  // ---- phase A: depthwise 3x3 -> dl, one channel group per round ----------
  dense_dw<FAST>(cp.dw, dv, mw + r16, mw + r16 < P, lane, r16, g, dl, L.S1);
  dense_wave_sync();

  // ---- phase B: first 1x1 (+ residual ADD) -> pl --------------------------
  {
    const bh_conv_params& a = cp.pw1;
    const int N1 = a.out_c;
    const int T1 = (N1 + 15) >> 4;
    const int KS1 = a.k_pad >> 6;
    const unsigned char* xrow = dl + r16 * L.S1 + g * 16;
    const uint8_t* res = (const uint8_t*)a.residual;
    const ResidualAdd A = residual_of(a);
    const DenseConv ac = dense_conv(a, r16, g);
    for (int t = 0; t < T1; ++t) {
      // rounds of two K-steps, each a load round of its own: the SIMD's other
      // waves cover it, and nothing is held across a round but the accumulator
      DenseTile<2> cur;
      dense_tile_load<2>(ac, t, 0, KS1, cur);
      v4i acc = (v4i){cur.be, cur.be, cur.be, cur.be};
      const int mu = cur.mu, sh = cur.sh;
      for (int k = 0;;) {
        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(*(const v4i*)(xrow + k * 64), cur.w[0], acc, 0, 0, 0);
        if (k + 1 < KS1)
          acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(*(const v4i*)(xrow + (k + 1) * 64), cur.w[1], acc, 0, 0, 0);
        k += 2;
        if (k >= KS1) break;
        dense_filter_load<2>(ac, t, k, KS1, cur.w);
      }
      const int n = t * 16 + r16;
      if (n < N1) {
        const ChanQ q = chan_q(mu, sh, a.out_zp);
        int32_t v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = requant_out<FAST>(acc[r], q, a.out_zp, a.act_min, a.act_max);
        if (res) {
          int32_t rq[4];
#pragma unroll
          for (int r = 0; r < 4; ++r)  // rows past P: a valid address, the value never stored
            rq[r] = (int32_t)(int8_t)res[(uint32_t)(min(mw + orow + r, P - 1) * N1 + n)];
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = residual_add_tab(add_tab, A, v[r], rq[r]);
        }
        stage4(pl, L.S2, orow, n, v);
      }
    }
    dense_wave_sync();
    if (a.output) dense_copy_rows(pl, L.S2, (uint8_t*)a.output + (long)mw * N1, N1, rows, lane);
  }
  if (!cp.has_pw2) return;

  // ---- phase C: second 1x1 from pl -> dl (row stride N2) -> HBM ------------
  {
    const bh_conv_params& b = cp.pw2;
    const int N2 = b.out_c;
    const int T2 = (N2 + 15) >> 4;
    const int KS2 = b.k_pad >> 6;
    v4i x[KX];
#pragma unroll
    for (int k = 0; k < KX; ++k) x[k] = k < KS2 ? *(const v4i*)(pl + r16 * L.S2 + g * 16 + k * 64) : (v4i){0, 0, 0, 0};
    // the next tile's round in flight behind this tile's MFMAs and epilogue
    // where the fragments are few (K <= 128)
    constexpr bool PF = KX <= 2;
    const DenseConv bc = dense_conv(b, r16, g);
    DenseTile<KX> cur, nxt;
    if (PF) dense_tile_load<KX>(bc, 0, 0, KS2, cur);
    for (int t = 0; t < T2; ++t) {
      if (!PF) dense_tile_load<KX>(bc, t, 0, KS2, cur);
      else if (t + 1 < T2) dense_tile_load<KX>(bc, t + 1, 0, KS2, nxt);
      v4i acc = (v4i){cur.be, cur.be, cur.be, cur.be};
#pragma unroll
      for (int k = 0; k < KX; ++k)
        if (k < KS2) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(x[k], cur.w[k], acc, 0, 0, 0);
      const int n = t * 16 + r16;
      if (n < N2) {
        const ChanQ q = chan_q(cur.mu, cur.sh, b.out_zp);
        int32_t v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = requant_out<FAST>(acc[r], q, b.out_zp, b.act_min, b.act_max);
        stage4(dl, N2, orow, n, v);
      }
      if (PF && t + 1 < T2) cur = nxt;
    }
    dense_wave_sync();
    dense_copy_rows(dl, N2, (uint8_t*)b.output + (long)mw * N2, N2, rows, lane);
  }
}

#ifndef BH_DENSE_WPE
#define BH_DENSE_WPE 8
#endif

template <bool FAST, int KX, int WPE>
static void launch_dense(const bh_chain_params& p, int P, const DenseLds& L, hipStream_t s) {
  ChainDivs dv;
  dv.out_w = FastDiv(p.dw.out_w);
  dv.out_h = FastDiv(p.dw.out_h);
  BH_LAUNCH((chain_dense_kernel<FAST, KX, WPE>), dim3((P + 63) / 64), dim3(256), L.bytes, s, p, P, L, dv);
}

}  // namespace bh

// LDS bytes of the dense form for these parameters, 0 when they do not admit
// it.  Called by bh_chain_lds_bytes after the checks every chain form shares.
extern "C" size_t bh_chain_dense_lds_bytes(const bh_chain_params* pp) {
  const bh_chain_params& p = *pp;
  if (p.dense != 1 || p.px_blocks != 4 || (p.waves != 0 && p.waves != 4)) return 0;
  if (p.tile || p.persist || p.deep || p.stage || p.c_split > 1) return 0;
  // 32-bit filter offsets in the kernel
  if ((long)p.pw1.n_pad * p.pw1.k_pad >= INT32_MAX || (p.has_pw2 && (long)p.pw2.n_pad * p.pw2.k_pad >= INT32_MAX)) return 0;
  const bh::DenseLds L = bh::dense_lds(p);
  return L.bytes <= 64 * 1024 ? L.bytes : 0;  // a form for many resident workgroups: no LDS opt-in
}

extern "C" int bh_chain_dense_launch(const bh_chain_params* pp, bh_stream_t stream) {
  const bh_chain_params& p = *pp;
  const int P = p.dw.batch * p.dw.out_h * p.dw.out_w;
  const bh::DenseLds L = bh::dense_lds(p);
  const bool fast = p.dw.requant_fast && p.pw1.requant_fast && (!p.has_pw2 || p.pw2.requant_fast);
  hipStream_t s = (hipStream_t)stream;
  const int ks2 = p.has_pw2 ? p.pw2.k_pad >> 6 : 1;
  if (ks2 <= 1) {
    if (fast) bh::launch_dense<true, 1, BH_DENSE_WPE>(p, P, L, s);
    else bh::launch_dense<false, 1, BH_DENSE_WPE>(p, P, L, s);
  } else if (ks2 <= 2) {
    if (fast) bh::launch_dense<true, 2, BH_DENSE_WPE>(p, P, L, s);
    else bh::launch_dense<false, 2, BH_DENSE_WPE>(p, P, L, s);
  } else {
    if (fast) bh::launch_dense<true, 5, BH_DENSE_WPE>(p, P, L, s);
    else bh::launch_dense<false, 5, BH_DENSE_WPE>(p, P, L, s);
  }
  return bh_check_launch("chain_dense_kernel");
}
