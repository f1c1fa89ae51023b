// Stand-alone driver of the hybrid CONV_2D / DEPTHWISE_CONV_2D host twins
// (backend/hip/cpu_kernels.h: CpuDynQuantItems, CpuConvHybrid,
// CpuDwConvHybrid) on a few launcher cases, each buffer sized exactly, against
// a plain restatement of the rule's integer sum and epilogue.  Built with
// -fsanitize=address,undefined by tests/test_conv_hybrid_cpu.py; links
// cpu_kernels.cc and quant.cc.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "backend/hip/cpu_kernels.h"

using namespace band::hip;

// CpuReindex's helper lives with the device kernels; nothing here reaches it
extern "C" int bh_reindex_canonical(const bh_reindex_params*, bh_reindex_params*) { return -1; }
// the pools here are not pinned
namespace band {
namespace hip {
bool PinThread(pthread_t, const std::vector<int>&) { return false; }
}  // namespace hip
}  // namespace band

namespace {

struct Case {
  int form;  // 0 CONV_2D one scale, 1 CONV_2D out_c scales, 2 DEPTHWISE_CONV_2D
  int batch, in_h, in_w, in_c, out_c, k_h, k_w, stride, dil, pad_h, pad_w, out_h, out_w, dm;
  bool bias;
};

uint32_t g_state = 12345u;
uint32_t Next() { return g_state = g_state * 1664525u + 1013904223u; }
float Uniform() { return static_cast<float>(Next() >> 8) / 8388608.0f - 1.0f; }

bool Run(const Case& c, int threads) {
  const bool dw = c.form == 2;
  const int K = c.k_h * c.k_w * (dw ? 1 : c.in_c);
  const int k_pad = (K + 15) / 16 * 16;
  const int item = c.in_h * c.in_w * c.in_c;
  std::vector<float> x(static_cast<size_t>(c.batch) * item);
  for (int b = 0; b < c.batch; ++b)
    for (int i = 0; i < item; ++i) x[static_cast<size_t>(b) * item + i] = Uniform() * (1.f + b) + (b == 1 ? 2.5f : 0.f);
  std::vector<int8_t> q(x.size());
  std::vector<float> s(c.batch), ws(c.out_c), bias(c.out_c);
  std::vector<int32_t> off(c.batch);
  std::vector<int8_t> w(dw ? static_cast<size_t>(K) * c.out_c : static_cast<size_t>(c.out_c) * k_pad, 0);
  for (int o = 0; o < c.out_c; ++o) {
    for (int k = 0; k < K; ++k)
      w[dw ? static_cast<size_t>(k) * c.out_c + o : static_cast<size_t>(o) * k_pad + k] =
          static_cast<int8_t>(static_cast<int>(Next() % 255u) - 127);
    ws[o] = c.form == 0 ? 0.0123f : 0.004f + 0.001f * o;
    bias[o] = Uniform();
  }
  CpuPool pool(threads);
  bh_dynquant_items_params d{};
  d.items = c.batch; d.item_size = item; d.asymmetric = c.form != 0;
  d.input = x.data(); d.q = q.data(); d.scale = s.data(); d.offset = off.data();
  CpuDynQuantItems(d, pool);
  std::vector<float> y(static_cast<size_t>(c.batch) * c.out_h * c.out_w * c.out_c, NAN);
  bh_conv_hybrid_params p{};
  p.batch = c.batch; p.in_h = c.in_h; p.in_w = c.in_w; p.in_c = c.in_c;
  p.out_h = c.out_h; p.out_w = c.out_w; p.out_c = c.out_c;
  p.k_h = c.k_h; p.k_w = c.k_w; p.stride_h = p.stride_w = c.stride; p.dil_h = p.dil_w = c.dil;
  p.pad_h = c.pad_h; p.pad_w = c.pad_w; p.k_pad = k_pad; p.depth_multiplier = c.dm; p.per_channel = c.form == 1;
  p.act_min = -INFINITY; p.act_max = 6.f;
  p.q = q.data(); p.in_scale = s.data(); p.in_offset = off.data();
  p.weights = w.data(); p.w_row_sum = nullptr; p.w_scale = ws.data();
  p.bias = c.bias ? bias.data() : nullptr; p.output = y.data();
  if (dw) CpuDwConvHybrid(p, pool); else CpuConvHybrid(p, pool);
  // the rule again, plainly
  for (int b = 0; b < c.batch; ++b) {
    if (c.form == 0 && off[b] != 0) return false;
    for (int oy = 0; oy < c.out_h; ++oy)
      for (int ox = 0; ox < c.out_w; ++ox)
        for (int o = 0; o < c.out_c; ++o) {
          long acc = 0;
          for (int ky = 0; ky < c.k_h; ++ky)
            for (int kx = 0; kx < c.k_w; ++kx) {
              const int iy = oy * c.stride - c.pad_h + ky * c.dil, ix = ox * c.stride - c.pad_w + kx * c.dil;
              if (iy < 0 || iy >= c.in_h || ix < 0 || ix >= c.in_w) continue;
              const int8_t* px = &q[((static_cast<size_t>(b) * c.in_h + iy) * c.in_w + ix) * c.in_c];
              if (dw) {
                acc += static_cast<long>(w[static_cast<size_t>(ky * c.k_w + kx) * c.out_c + o]) * (px[o / c.dm] - off[b]);
              } else {
                for (int ci = 0; ci < c.in_c; ++ci)
                  acc += static_cast<long>(w[static_cast<size_t>(o) * k_pad + (ky * c.k_w + kx) * c.in_c + ci]) * (px[ci] - off[b]);
              }
            }
          const float bv = c.bias ? bias[o] : 0.f;
          volatile float a, t, v;
          if (c.form == 1) {
            a = static_cast<float>(acc) * ws[o]; t = a * s[b]; v = t + bv;
          } else {
            a = s[b] * ws[o]; t = static_cast<float>(acc) * a; v = bv + t;
          }
          const float want = std::fmin(v, 6.f);
          const float got = y[((static_cast<size_t>(b) * c.out_h + oy) * c.out_w + ox) * c.out_c + o];
          if (!(got == want)) {
            std::printf("form %d b %d (%d, %d) c %d: got %.9g want %.9g\n", c.form, b, oy, ox, o, got, want);
            return false;
          }
        }
  }
  return true;
}

}  // namespace

int main() {
  const Case cases[] = {
      {0, 2, 5, 6, 5, 7, 3, 3, 1, 1, 1, 1, 5, 6, 1, true},     // 3x3 SAME
      {1, 3, 7, 6, 3, 17, 3, 3, 2, 1, 1, 0, 4, 3, 1, false},   // stride 2, the asymmetric pad
      {1, 2, 9, 8, 4, 5, 3, 3, 1, 2, 2, 2, 9, 8, 1, true},     // dilation 2
      {1, 1, 1, 1, 1280, 33, 1, 1, 1, 1, 0, 0, 1, 1, 1, true}, // the head
      {2, 2, 5, 6, 5, 10, 3, 3, 1, 1, 1, 1, 5, 6, 2, true},    // depth multiplier 2
      {2, 3, 7, 7, 12, 12, 5, 5, 2, 1, 2, 2, 4, 4, 1, false},  // 5x5 stride 2
  };
  int n = 0;
  for (const Case& c : cases)
    for (int threads : {1, 3}) {
      if (!Run(c, threads)) return 1;
      ++n;
    }
  std::printf("%d cases ok\n", n);
  return 0;
}
