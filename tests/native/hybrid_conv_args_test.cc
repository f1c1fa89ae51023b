// Stand-alone driver of HybridConvArgs (backend/hip/lower_args.h): parses the
// .tflite files named on the command line and classifies every hybrid CONV_2D
// / DEPTHWISE_CONV_2D, printing the form, the quantisation, the geometry and
// the first and last expanded scale, or the reason it is refused.  Built with
// -fsanitize=address,undefined by tests/test_lower_args_hybrid_conv_cpu.py;
// links only tflite_reader.cc, lower_args.cc, quant.cc and
// compat/band/common.cc.
#include <cstdio>
#include <string>
#include <vector>

#include "backend/hip/lower_args.h"

using namespace band::hip;

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    std::vector<uint8_t> bytes;
    FILE* f = std::fopen(argv[a], "rb");
    if (!f) {
      std::printf("%s: cannot open\n", argv[a]);
      return 2;
    }
    uint8_t chunk[4096];
    for (size_t n; (n = std::fread(chunk, 1, sizeof(chunk), f)) > 0;) bytes.insert(bytes.end(), chunk, chunk + n);
    std::fclose(f);
    TflModel m;
    std::string err;
    if (!m.Parse(bytes.data(), bytes.size(), &err)) {
      std::printf("%s: %s\n", argv[a], err.c_str());
      return 2;
    }
    for (size_t i = 0; i < m.ops.size(); ++i) {
      const TflOperator& op = m.ops[i];
      if (!ex::IsHybridConvOp(m, op)) {
        std::printf("%s op %zu %s: not hybrid\n", argv[a], i, TflBuiltinName(op.builtin));
        continue;
      }
      ex::HybridConvGeometry g;
      const char* why = "refused";
      const char* pure = "refused";
      const bool ok = ex::HybridConvArgs(m, op, &g, &why);
      if (ex::HybridConvArgs(m, op, nullptr, &pure) != ok) return 3;  // the pure check agrees
      if (!ok) {
        std::printf("%s op %zu %s: %s\n", argv[a], i, TflBuiltinName(op.builtin), why);
        continue;
      }
      const ex::ConvGeometry& c = g.conv;
      if (g.w_scale.size() != static_cast<size_t>(c.out_c)) return 4;
      std::printf("%s op %zu %s: ok %s %s in %dx%dx%dx%d out %dx%dx%d k %dx%d stride %d dil %d pad %d,%d dm %d act %d bias %d "
                  "scales %.9g %.9g\n",
                  argv[a], i, TflBuiltinName(op.builtin), g.depthwise ? "depthwise" : "conv",
                  g.per_channel ? "per_channel asymmetric" : "per_tensor symmetric", c.batch, c.in_h, c.in_w, c.in_c,
                  c.out_h, c.out_w, c.out_c, c.k_h, c.k_w, c.stride_h, c.dil_h, c.pad_h, c.pad_w, c.depth_multiplier, c.act,
                  c.bias >= 0 ? 1 : 0, g.w_scale.front(), g.w_scale.back());
    }
  }
  return 0;
}
