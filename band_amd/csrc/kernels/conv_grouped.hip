// Grouped CONV_2D for gfx950 (filter [oc][kh][kw][icg] with icg != in_c):
// reference_integer_ops::ConvPerChannel / reference_ops::Conv with
// groups = in_c / icg.  Output channel c belongs to group c / ocg
// (ocg = oc / groups) and contracts over K_g = kh*kw*icg bytes of that
// group's channel slice [g*icg, (g+1)*icg) of every tap; bias, multipliers,
// zero points and clamp are the dense op's, indexed by the total channel.
//
// One launch, work proportional to K_g.  The packed filters are the dense
// ones with K = K_g (bh_pack_conv_weights: one K_g-byte row per output
// channel, bias_eff folded over K_g), so group g owns rows [g*ocg, (g+1)*ocg).
//
// conv_grouped_mfma_kernel: a wave owns WM pixel tiles x one 16-channel tile
// at a 16-aligned TOTAL channel n0, transposed as in conv_mfma_kernel
// (D^T = W x X^T on v_mfma_i32_16x16x64_i8: lane (q, r) supplies filter row
// n0 + r and pixel r at k = 16q .. 16q+15 and ends up with channels
// n0 + 4q .. +3 of pixel r), so the dense epilogue's dword store is used
// unchanged whatever ocg is.  The tile's K axis is the concatenation of its
// groups' K_g, each padded to 16 bytes: 16-byte chunk c belongs to group
// g_lo + c / cpg at k offset 16 * (c % cpg) (cpg = ceil(K_g / 16)), and lane
// group q of K-step s holds chunk 4s + q.  A lane's A fragment is gathered
// from that chunk's group slice (pixel stride in_c, zero past K_g, the input
// zero point on padding taps); its B fragment is its filter row's 16 bytes
// when the row's channel is in the chunk's group and zero otherwise - the
// block-diagonal placement inside one MFMA tile.  A tile inside one group
// (ocg % 16 == 0) walks K_g once; a tile over several small groups packs
// them 16 bytes apart, so e.g. four 36-byte groups take 3 K-steps, not 4.
//
// uint8 filters (w_zp != 0) need sum_k x'[m][k] over the channel's own group:
// a second MFMA per step with B = 1 on the same block-diagonal mask gives it
// per (channel, pixel) in the accumulator layout.
#include <cstdlib>

#include "common.hpp"
#include "conv_epilogue.hpp"

namespace bh {

struct GroupedGeom {
  int icg, ocg, kg, cpg;  // channels per group (in / out), K_g, 16-byte chunks per group
  FastDiv out_w, out_h, icg_d, k_w, cpg_d, ocg_d;
};

constexpr int GKU = 2;  // K-steps whose loads are issued together

// 16 int8-domain A bytes of im2col row `ri` in group `grp`, k in [kc, kc+16)
template <bool IS1X1, int VEC>
__device__ __forceinline__ v4i gather_a(const bh_conv_params& p, const GroupedGeom& gg, const RowInfo& ri, int grp,
                                        int kc, uint32_t xorw, uint32_t padw) {
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  if (ri.valid) {
    const uint8_t* in = (const uint8_t*)p.input + ri.base + (long)grp * gg.icg;
#pragma unroll
    for (int u = 0; u < 16 / VEC; ++u) {
      const int k = kc + u * VEC;
      if (k < gg.kg) {
        if constexpr (IS1X1) {
          load_unit<VEC>(in + k, w, u);
          xor_unit<VEC>(w, u, xorw);
        } else {
          const int tap = gg.icg_d.div(k);
          const int ci = k - tap * gg.icg;
          const int fy = gg.k_w.div(tap);
          const int fx = tap - fy * p.k_w;
          const int y = ri.y0 + fy * p.dil_h;
          const int x = ri.x0 + fx * p.dil_w;
          if (y >= 0 && y < p.in_h && x >= 0 && x < p.in_w) {
            load_unit<VEC>(in + ((long)y * p.in_w + x) * p.in_c + ci, w, u);
            xor_unit<VEC>(w, u, xorw);
          } else {
            fill_unit<VEC>(w, u, padw);
          }
        }
      }
    }
  }
  v4i r;
  r.x = (int)w[0]; r.y = (int)w[1]; r.z = (int)w[2]; r.w = (int)w[3];
  return r;
}

template <int WM, bool IS1X1, int VEC>
__global__ __launch_bounds__(256) void conv_grouped_mfma_kernel(bh_conv_params p, GroupedGeom gg, int M, int N,
                                                                int gn) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  // channel tiles fastest: neighbouring workgroups read the same pixels
  const int bm = (int)blockIdx.x / gn;
  const int bn = (int)blockIdx.x - bm * gn;
  const int m0 = (bm * 4 + wave) * WM * 16;
  const int n0 = bn * 16;
  if (m0 >= M) return;  // whole wave; the kernel has no barrier
  const int r16 = lane & 15;
  const int q = lane >> 4;
  const bool wzp = p.w_zp != 0;
  const uint32_t xorw = splat_byte(p.in_xor);
  const uint32_t padw = splat_byte(p.in_zp);

  RowInfo ri[WM];
#pragma unroll
  for (int wm = 0; wm < WM; ++wm) {
    const int m = m0 + wm * 16 + r16;
    ri[wm].valid = m < M;
    const int mm = ri[wm].valid ? m : 0;
    const int t = gg.out_w.div(mm);
    const int ox = mm - t * p.out_w;
    const int n = gg.out_h.div(t);
    const int oy = t - n * p.out_h;
    if constexpr (IS1X1) {
      ri[wm].base = (((long)n * p.in_h + (long)oy * p.stride_h) * p.in_w + (long)ox * p.stride_w) * p.in_c;
      ri[wm].y0 = 0; ri[wm].x0 = 0;
    } else {
      ri[wm].base = (long)n * p.in_h * p.in_w * p.in_c;
      ri[wm].y0 = oy * p.stride_h - p.pad_h;
      ri[wm].x0 = ox * p.stride_w - p.pad_w;
    }
  }

  // this lane's filter row and its group; the groups the tile touches
  const int ch = n0 + r16;
  const int my_grp = ch < N ? (int)gg.ocg_d.div(ch) : -1;
  const int g_lo = gg.ocg_d.div(n0);
  const int g_hi = gg.ocg_d.div(min(n0 + 15, N - 1));
  const int chunks = (g_hi - g_lo + 1) * gg.cpg;
  const int steps = (chunks + 3) >> 2;
  const int8_t* wrow = p.weights + (long)ch * p.k_pad;  // ch < n_pad: n_pad % 64 == 0

  v4i acc[WM], rs[WM];
#pragma unroll
  for (int i = 0; i < WM; ++i) {
    acc[i] = (v4i){0, 0, 0, 0};
    rs[i] = (v4i){0, 0, 0, 0};
  }

  for (int s0 = 0; s0 < steps; s0 += GKU) {
    v4i a[GKU][WM], b[GKU], ones[GKU];
#pragma unroll
    for (int u = 0; u < GKU; ++u) {
      const int c = (s0 + u) * 4 + q;
      const bool live = c < chunks;
      const int gi = gg.cpg_d.div(live ? c : 0);
      const int kc = ((live ? c : 0) - gi * gg.cpg) * 16;
      const int grp = g_lo + gi;
      const bool mine = live && grp == my_grp;
#pragma unroll
      for (int wm = 0; wm < WM; ++wm)
        a[u][wm] = live ? gather_a<IS1X1, VEC>(p, gg, ri[wm], grp, kc, xorw, padw) : (v4i){0, 0, 0, 0};
      b[u] = mine ? *(const v4i*)(wrow + kc) : (v4i){0, 0, 0, 0};
      const int one = mine ? 0x01010101 : 0;
      ones[u] = (v4i){one, one, one, one};
    }
#pragma unroll
    for (int u = 0; u < GKU; ++u) {
      if (s0 + u < steps) {
#pragma unroll
        for (int wm = 0; wm < WM; ++wm) {
          acc[wm] = __builtin_amdgcn_mfma_i32_16x16x64_i8(b[u], a[u][wm], acc[wm], 0, 0, 0);
          if (wzp) rs[wm] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones[u], a[u][wm], rs[wm], 0, 0, 0);
        }
      }
    }
  }

  const int nb = n0 + 4 * q;
  if (nb >= N) return;
  const Chan4 c4 = chan4(p, nb, N);
#pragma unroll
  for (int wm = 0; wm < WM; ++wm) {
    v4i v = acc[wm];
    // the per-channel row-sum term here (a dword of channels may span
    // groups); conv_store4's own per-pixel term then sees rsum = 0
    if (wzp) {
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] -= p.w_zp * rs[wm][r];
    }
    conv_store4(p, v, 0, m0 + wm * 16 + r16, nb, M, N, c4);
  }
}

template <int WM, bool IS1X1, int VEC>
static int launch_grouped(const bh_conv_params& p, const GroupedGeom& gg, int M, int N, hipStream_t s) {
  const int gn = (N + 15) / 16;
  const long gm = ((long)M + 64 * WM - 1) / (64 * WM);
  BH_LAUNCH((conv_grouped_mfma_kernel<WM, IS1X1, VEC>), dim3((unsigned)(gm * gn)), dim3(256), 0, s, p, gg, M, N, gn);
  return bh_check_launch("conv_grouped_mfma_kernel");
}

template <bool IS1X1, int VEC>
static int launch_grouped_wm(const bh_conv_params& p, const GroupedGeom& gg, int M, int N, hipStream_t s) {
  // Routing (profiles/r13a_grouped_conv.json, `forms`): one 16-pixel tile
  // per wave.  Two tiles per wave (each filter fragment feeds two MFMAs) are
  // 0.88 - 2.92 us slower on every batch-1 layer of ShuffleNet-v1 g=3 and
  // ResNeXt-50 32x4d, and 0.23 - 1.40 us slower on 8 of the 10 layers at
  // batch 24; the two they win (ResNeXt 14x14 by 0.52 us, ShuffleNet stage
  // 3's second pointwise by 0.15 us, both M = 4704) share their M with a
  // layer they lose by 1.19 us (stage 3's first pointwise), so no rule on
  // M separates them.  They stay reachable by hint.
  if (p.kernel_hint == BH_CONV_GROUPED_MFMA_2) return launch_grouped<2, IS1X1, VEC>(p, gg, M, N, s);
  return launch_grouped<1, IS1X1, VEC>(p, gg, M, N, s);
}

}  // namespace bh

namespace {
// validated geometry of a grouped layer; false: the block is not runnable
bool grouped_geom(const bh_conv_grouped_params* gp, bh::GroupedGeom* gg, long* Ml) {
  if (!gp) return false;
  const bh_conv_params& p = gp->conv;
  const int G = gp->groups;
  if (G < 1 || p.in_c <= 0 || p.out_c <= 0 || p.in_c % G || p.out_c % G) return false;
  if (p.k_h <= 0 || p.k_w <= 0 || p.stride_h <= 0 || p.stride_w <= 0 || p.dil_h <= 0 || p.dil_w <= 0) return false;
  const long kg = (long)p.k_h * p.k_w * (p.in_c / G);
  *Ml = (long)p.batch * p.out_h * p.out_w;
  if (*Ml <= 0 || *Ml > INT32_MAX || kg > INT32_MAX / 2 || p.k_pad < kg || p.n_pad < p.out_c || (p.k_pad % 64) ||
      (p.n_pad % 64) || !p.input || !p.output || !p.weights || !p.bias_eff || !p.mult || !p.shift ||
      p.out_img_stride < 0)
    return false;
  if ((long)p.batch * p.in_h * p.in_w <= 0) return false;
  // 1-D grid of 64-pixel x 16-channel workgroups
  if ((*Ml + 63) / 64 * ((p.out_c + 15) / 16) > INT32_MAX) return false;
  gg->icg = p.in_c / G;
  gg->ocg = p.out_c / G;
  gg->kg = (int)kg;
  gg->cpg = (int)((kg + 15) / 16);
  gg->out_w = bh::FastDiv(p.out_w);
  gg->out_h = bh::FastDiv(p.out_h);
  gg->icg_d = bh::FastDiv(gg->icg);
  gg->k_w = bh::FastDiv(p.k_w);
  gg->cpg_d = bh::FastDiv(gg->cpg);
  gg->ocg_d = bh::FastDiv(gg->ocg);
  return true;
}
}  // namespace

extern "C" const char* bh_conv2d_grouped_i8_kernel(const bh_conv_grouped_params* gp) {
  bh::GroupedGeom gg;
  long M = 0;
  // one form is built (BH_CONV_GROUPED_MFMA_2 widens its pixel tile); BH_CONV_GROUPED_AUTO routes to it
  return grouped_geom(gp, &gg, &M) ? "conv_grouped_mfma_kernel" : "";
}

extern "C" int bh_conv2d_grouped_i8(const bh_conv_grouped_params* gp, bh_stream_t stream) {
  bh::GroupedGeom gg;
  long Ml = 0;
  if (!grouped_geom(gp, &gg, &Ml)) {
    bh_set_last_error("bh_conv2d_grouped_i8: invalid parameters");
    return BH_EINVAL;
  }
  const bh_conv_params& p = gp->conv;
  const int M = (int)Ml, N = p.out_c;
  hipStream_t s = (hipStream_t)stream;
  const bool is1x1 = p.k_h == 1 && p.k_w == 1 && p.pad_h == 0 && p.pad_w == 0;
  // widest fragment unit the group slices allow: slice g of a pixel starts at
  // byte g * icg of it, so icg (hence in_c) and the tensor base decide
  const uintptr_t al = (uintptr_t)p.input | (uintptr_t)gg.icg;
  if (is1x1) {
    if (al % 16 == 0) return bh::launch_grouped_wm<true, 16>(p, gg, M, N, s);
    if (al % 8 == 0) return bh::launch_grouped_wm<true, 8>(p, gg, M, N, s);
    if (al % 4 == 0) return bh::launch_grouped_wm<true, 4>(p, gg, M, N, s);
    return bh::launch_grouped_wm<true, 1>(p, gg, M, N, s);
  }
  if (al % 16 == 0) return bh::launch_grouped_wm<false, 16>(p, gg, M, N, s);
  if (al % 8 == 0) return bh::launch_grouped_wm<false, 8>(p, gg, M, N, s);
  if (al % 4 == 0) return bh::launch_grouped_wm<false, 4>(p, gg, M, N, s);
  return bh::launch_grouped_wm<false, 1>(p, gg, M, N, s);
}
