// Stand-alone driver of CpuGather (backend/hip/cpu_kernels.h), the host twin of
// bh_gather: every buffer sized exactly, so that a read of a row the range
// check should have refused, or a write past the output, is a sanitizer
// report.  int32 and int64 indices, 1- and 4-byte elements, in-range rows,
// the extreme indices and a refused block.  Built with
// -fsanitize=address,undefined by tests/test_gather_cpu.py; links
// cpu_kernels.cc and quant.cc.
#include <cstdint>
#include <cstdio>
#include <cstring>
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

int g_failed = 0;
#define CHECK(cond)                                          \
  do {                                                       \
    if (!(cond)) {                                           \
      std::printf("FAIL line %d: %s\n", __LINE__, #cond);    \
      ++g_failed;                                            \
    }                                                        \
  } while (0)

template <typename Index>
void Run(int elem_bytes, int64_t outer, int64_t axis_size, int64_t inner, const std::vector<Index>& idx) {
  const size_t row = static_cast<size_t>(inner) * elem_bytes;
  std::vector<uint8_t> table(static_cast<size_t>(outer * axis_size) * row);
  for (size_t i = 0; i < table.size(); ++i) table[i] = static_cast<uint8_t>(1 + (7 * i + 3) % 170);
  std::vector<uint8_t> out(static_cast<size_t>(outer) * idx.size() * row, 0xff);
  // 4-byte elements: vectors of uint8_t come from operator new, aligned to 16
  bh_gather_params p{};
  p.elem_bytes = elem_bytes;
  p.index_bytes = static_cast<int>(sizeof(Index));
  p.outer = outer;
  p.axis_size = axis_size;
  p.n_idx = static_cast<int64_t>(idx.size());
  p.inner = inner;
  p.params = table.data();
  p.indices = idx.data();
  p.output = out.data();
  CHECK(CpuGather(p));
  for (int64_t o = 0; o < outer; ++o) {
    for (size_t j = 0; j < idx.size(); ++j) {
      const uint8_t* got = out.data() + (static_cast<size_t>(o) * idx.size() + j) * row;
      const bool ok = idx[j] >= 0 && static_cast<int64_t>(idx[j]) < axis_size;
      for (size_t b = 0; b < row; ++b) {
        const uint8_t want = ok ? table[static_cast<size_t>(o * axis_size + static_cast<int64_t>(idx[j])) * row + b] : 0;
        if (got[b] != want) {
          std::printf("FAIL elem_bytes %d outer %lld index %lld byte %zu\n", elem_bytes, static_cast<long long>(o),
                      static_cast<long long>(idx[j]), b);
          ++g_failed;
          return;
        }
      }
    }
  }
}

}  // namespace

int main() {
  const std::vector<int32_t> i32 = {0, 8, 3, 3, INT32_MIN, 5, INT32_MAX, -1, 9, 8};
  const std::vector<int64_t> i64 = {0, 8, (1ll << 32) + 1, 1, -(1ll << 32) + 2, 2, 1ll << 40, INT64_MIN, INT64_MAX, -1, 9, 8};
  for (int eb : {1, 4}) {
    for (int64_t inner : {1, 3, 4, 16, 260}) {
      Run<int32_t>(eb, 1, 9, inner, i32);
      Run<int64_t>(eb, 1, 9, inner, i64);
      Run<int32_t>(eb, 3, 9, inner, i32);
      Run<int64_t>(eb, 3, 9, inner, i64);
    }
  }
  Run<int32_t>(1, 2, 1, 12, {0, 0, 1, -1});
  bh_gather_params bad{};
  CHECK(!CpuGather(bad));
  std::printf("%s\n", g_failed ? "FAILED" : "gather twin ok");
  return g_failed ? 1 : 0;
}
