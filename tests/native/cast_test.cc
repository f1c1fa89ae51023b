// Stand-alone driver of CAST's host code: CpuCast (cpu_kernels.cc, the
// conversion of band_hip_cast_shared.h) over the 16 type pairs on exactly
// sized heap buffers that lie one byte off their allocation, with NaN, the
// infinities, +-2^31, +-2^63 and -0.5 among the float sources and the extremes
// among the integer ones, checked against the rule spelt out here; and
// CastArgs (lower_args.cc) on the .tflite files named on the command line,
// printing "ok" or the reason.  Built with -fsanitize=address,undefined by
// tests/test_cast_mask_cpu.py; links tflite_reader.cc, lower_args.cc,
// quant.cc, cpu_kernels.cc and compat/band/common.cc.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "backend/hip/cpu_kernels.h"
#include "backend/hip/lower_args.h"

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

int g_failed = 0;

template <class S>
std::vector<S> Sources();
template <>
std::vector<float> Sources<float>() {
  const float inf = std::numeric_limits<float>::infinity();
  return {std::numeric_limits<float>::quiet_NaN(), inf, -inf, 2147483648.0f, -2147483648.0f, 9223372036854775808.0f,
          -9223372036854775808.0f, -0.5f, 0.5f, -0.0f, 255.9f, 256.0f, -1.0f, 3.0e38f, -3.0e38f, 1.0e-45f, 100.7f, -100.7f};
}
template <>
std::vector<uint8_t> Sources<uint8_t>() { return {0, 1, 127, 128, 255}; }
template <>
std::vector<int32_t> Sources<int32_t>() { return {0, 1, -1, 255, 256, 16777217, INT32_MAX, INT32_MIN}; }
template <>
std::vector<int64_t> Sources<int64_t>() {
  return {0, 1, -1, 255, 256, 4294967301LL, -4294967291LL, 9007199254740993LL, INT64_MAX, INT64_MIN};
}

// float32 -> integer by the rule, in long double (exact for every float)
template <class D>
D Expect(float f) {
  if (std::isnan(f)) return 0;
  const long double lo = std::numeric_limits<D>::min(), hi = std::numeric_limits<D>::max();
  const long double t = std::trunc(static_cast<long double>(f));
  return t <= lo ? std::numeric_limits<D>::min() : t >= hi ? std::numeric_limits<D>::max() : static_cast<D>(t);
}

template <class S, class D>
void Run(int in_type, int out_type) {
  const std::vector<S> src = Sources<S>();
  for (size_t n = 0; n <= src.size(); ++n) {
    std::unique_ptr<uint8_t[]> in(new uint8_t[1 + n * sizeof(S)]), out(new uint8_t[1 + n * sizeof(D)]);
    if (n) std::memcpy(in.get() + 1, src.data(), n * sizeof(S));
    CpuCast(bh_cast_params{in_type, out_type, static_cast<long>(n), in.get() + 1, out.get() + 1});
    if constexpr (std::is_same<S, float>::value && !std::is_same<D, float>::value) {
      for (size_t i = 0; i < n; ++i) {
        D got;
        std::memcpy(&got, out.get() + 1 + i * sizeof(D), sizeof(D));
        if (got != Expect<D>(src[i])) {
          std::printf("cast %d -> %d of %g: %lld\n", in_type, out_type, static_cast<double>(src[i]), static_cast<long long>(got));
          ++g_failed;
        }
      }
    }
  }
}

template <class S>
void RunFrom(int in_type) {
  Run<S, uint8_t>(in_type, BH_CAST_U8);
  Run<S, int32_t>(in_type, BH_CAST_I32);
  Run<S, int64_t>(in_type, BH_CAST_I64);
  Run<S, float>(in_type, BH_CAST_F32);
}

}  // namespace

int main(int argc, char** argv) {
  RunFrom<uint8_t>(BH_CAST_U8);
  RunFrom<int32_t>(BH_CAST_I32);
  RunFrom<int64_t>(BH_CAST_I64);
  RunFrom<float>(BH_CAST_F32);
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
      if (m.ops[i].builtin != kTflCast) continue;
      const char* why = "refused";
      int from = 0, to = 0;
      const bool ok = ex::CastArgs(m, m.ops[i], &from, &to, &why);
      std::printf("%s op %zu %s: %s\n", argv[a], i, TflBuiltinName(m.ops[i].builtin), ok ? "ok" : why);
    }
  }
  if (g_failed) return 1;
  std::printf("cast ok\n");
  return 0;
}
