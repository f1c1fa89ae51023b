// Prints what quant.cc derives for the LayerNorm / GELU ops, for
// tests/test_layernorm_cpu.py to compare with its numpy restatements.  Linked
// with quant.cc alone.  One request per argument group:
//   rsqrt <s_in> <z_in> <s_out> <z_out>                  -> 256 table bytes
//   gelu <signed> <approximate> <s_in> <z_in> <s_out> <z_out> -> 256 table bytes
//   sqdiff <s1> <s2> <s_out>                             -> m1 s1 m2 s2 mo so left_shift, or "refused: <why>"
//   invsqrt <v>                                          -> multiplier shift
// Scales are C hex floats (float.hex() of the float32 value).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "backend/hip/quant.h"

using namespace band::hip;

int main(int argc, char** argv) {
  int a = 1;
  auto f = [&]() { return std::strtof(argv[a++], nullptr); };
  auto i = [&]() { return static_cast<int>(std::strtol(argv[a++], nullptr, 10)); };
  while (a < argc) {
    const char* what = argv[a++];
    uint8_t table[256];
    bool is_table = false;
    if (!std::strcmp(what, "rsqrt") && a + 4 <= argc) {
      const float s_in = f();
      const int z_in = i();
      const float s_out = f();
      const int z_out = i();
      if (!RsqrtTable(s_in, z_in, s_out, z_out, table)) {
        std::printf("refused\n");
        continue;
      }
      is_table = true;
    } else if (!std::strcmp(what, "gelu") && a + 6 <= argc) {
      const int sg = i(), approx = i();
      const float s_in = f();
      const int z_in = i();
      const float s_out = f();
      const int z_out = i();
      GeluTable(sg != 0, approx != 0, s_in, z_in, s_out, z_out, table);
      is_table = true;
    } else if (!std::strcmp(what, "sqdiff") && a + 3 <= argc) {
      const float s1 = f(), s2 = f(), so = f();
      AddParams p;
      const char* why = "";
      if (SquaredDifferenceParams(s1, s2, so, &p, &why))
        std::printf("%d %d %d %d %d %d %d\n", p.m1, p.s1, p.m2, p.s2, p.mo, p.so, p.left_shift);
      else
        std::printf("refused: %s\n", why);
    } else if (!std::strcmp(what, "invsqrt") && a + 1 <= argc) {
      int32_t m;
      int e;
      GetInvSqrtQuantizedMultiplierExp(i(), -1, &m, &e);
      std::printf("%d %d\n", m, e);
    } else {
      std::printf("bad request %s\n", what);
      return 2;
    }
    if (is_table) {
      for (int k = 0; k < 256; ++k) std::printf("%d%c", table[k], k == 255 ? '\n' : ' ');
    }
  }
  return 0;
}
