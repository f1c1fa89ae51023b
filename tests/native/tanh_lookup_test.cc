// Stand-alone driver of the host code of TANH and EMBEDDING_LOOKUP: TanhTable
// (quant.cc) over a few quantisations into exactly sized tables, CpuUnaryF32's
// BH_UNARY_TANH (cpu_kernels.cc) on exactly sized heap buffers, the extremes
// among the inputs, and TanhArgs / EmbeddingLookupArgs (lower_args.cc) on the
// .tflite files named on the command line, printing "ok" or the reason.  Built
// with -fsanitize=address,undefined by tests/test_cast_tanh_cpu.py; links
// tflite_reader.cc, lower_args.cc, quant.cc, cpu_kernels.cc and
// compat/band/common.cc.
#include <cmath>
#include <cstdio>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "backend/hip/cpu_kernels.h"
#include "backend/hip/lower_args.h"
#include "backend/hip/quant.h"

using namespace band::hip;

// CpuReindex's helper lives with the device kernels; nothing here reaches it
extern "C" int bh_reindex_canonical(const bh_reindex_params*, bh_reindex_params*) { return -1; }
// the pools here are not pinned
namespace band {
namespace hip {
bool PinThread(pthread_t, const std::vector<int>&) { return false; }
}  // namespace hip
}  // namespace band

int main(int argc, char** argv) {
  const float scales[] = {0.004f, 0.05f, 0.25f, 3.0e38f, 1.0e-38f};
  for (int is_signed = 0; is_signed < 2; ++is_signed)
    for (float s : scales) {
      std::unique_ptr<uint8_t[]> table(new uint8_t[256]);
      TanhTable(is_signed != 0, s, is_signed ? -128 : 255, 1.0f / 128.0f, is_signed ? 0 : 128, table.get());
      TanhTable(is_signed != 0, s, is_signed ? 127 : 0, 1.0f / 256.0f, is_signed ? -128 : 0, table.get());
    }
  const float inf = std::numeric_limits<float>::infinity();
  const std::vector<float> x = {0.0f, -0.0f, 1.0f, -1.0f, 88.0f, -88.0f, 3.0e38f, -3.0e38f, 1.0e-45f, inf, -inf,
                                std::numeric_limits<float>::quiet_NaN()};
  for (size_t n = 0; n <= x.size(); ++n) {
    std::unique_ptr<float[]> in(new float[n ? n : 1]), out(new float[n ? n : 1]);
    for (size_t i = 0; i < n; ++i) in[i] = x[i];
    CpuUnaryF32(BH_UNARY_TANH, in.get(), out.get(), static_cast<long>(n), 0.f, 0.f);
    for (size_t i = 0; i < n; ++i)
      if (!(std::isnan(x[i]) ? std::isnan(out[i]) : std::fabs(out[i]) <= 1.0f)) {
        std::printf("tanh(%g) = %g\n", x[i], out[i]);
        return 1;
      }
  }
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
      const char* why = "refused";
      bool ok = false, batch_ok = false, is_float = false;
      if (op.builtin == kTflTanh) {
        ok = ex::TanhArgs(m, op, &is_float, &why);
      } else if (op.builtin == kTflEmbeddingLookup) {
        bh_gather_params p;
        ok = ex::EmbeddingLookupArgs(m, op, &p, &why, &batch_ok);
      } else {
        continue;
      }
      std::printf("%s op %zu %s: %s\n", argv[a], i, TflBuiltinName(op.builtin), ok ? "ok" : why);
    }
  }
  std::printf("tanh lookup ok\n");
  return 0;
}
