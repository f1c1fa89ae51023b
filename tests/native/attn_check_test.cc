// Stand-alone driver of bh_attention_i8's parameter check
// (band_hip_attention_shared.h, pure host code): a valid block with and
// without a bias, every refusal by reason, and hostile strides and extents
// (INT64_MAX, INT64_MIN, INT32_MAX) in every stride field, under
// -fsanitize=address,undefined (tests/test_attention_mask_cpu.py).  Links
// nothing of the project.
#include <cstdio>
#include <cstring>

#include "band_hip_attention_shared.h"

namespace {

int g_failed = 0;

bh_attention_params Valid(bool bias) {
  static float table[256];
  static int8_t buf[4096];
  bh_attention_params p{};
  p.batch[0] = 1; p.batch[1] = 2; p.rows = 5; p.keys = 7; p.head_dim = 16; p.out_dim = 16;
  p.q_bstride[1] = 80; p.k_bstride[1] = 112; p.v_bstride[1] = 112; p.out_bstride[1] = 80;
  p.q_row_stride = p.k_row_stride = p.v_row_stride = p.out_row_stride = 16;
  p.q_inner_stride = p.k_inner_stride = p.v_inner_stride = p.out_inner_stride = 1;
  p.qk.mult = p.pv.mult = 1 << 30; p.qk.shift = p.pv.shift = -3;
  p.table = table; p.q = p.k = p.v = buf; p.out = buf;
  if (bias) {
    p.bias = buf; p.bias_bstride[1] = 35; p.bias_row_stride = 7; p.bias_key_stride = 1;
    p.add.left_shift = 20; p.add.a_mult = p.add.b_mult = p.add.o_mult = 1 << 30;
    p.add.a_shift = p.add.b_shift = -1; p.add.o_shift = -19; p.add.act_min = -128; p.add.act_max = 127;
  }
  return p;
}

void Expect(const bh_attention_params& p, const char* fragment, const char* what) {
  const char* why = bh_attention_why(&p);
  const bool ok = fragment ? (why && std::strstr(why, fragment)) : !why;
  if (!ok) {
    std::printf("%s: %s\n", what, why ? why : "accepted");
    ++g_failed;
  }
}

}  // namespace

int main() {
  Expect(Valid(false), nullptr, "valid");
  Expect(Valid(true), nullptr, "valid with a bias");
  if (!bh_attention_why(nullptr)) ++g_failed;
  bh_attention_params p = Valid(true);
  p.bias_row_stride = -7; Expect(p, "negative bias stride", "row stride");
  p = Valid(true); p.bias_key_stride = 2; Expect(p, "key stride other than 0 or 1", "key stride");
  p = Valid(true); p.batch[1] = 65535; p.bias_bstride[1] = 1LL << 31; Expect(p, "2^31", "bias span");
  p = Valid(true); p.add.a_shift = 1; Expect(p, "ADD input shift above 0", "a_shift");
  p = Valid(true); p.add.o_shift = -32; Expect(p, "ADD shift outside", "o_shift");
  p = Valid(true); p.add.left_shift = 32; Expect(p, "left_shift outside 0 .. 31", "left_shift");
  p = Valid(true); p.add.act_min = 5; p.add.act_max = 4; Expect(p, "act_min > act_max", "window");
  p = Valid(true); p.add_scores_operand = 2; Expect(p, "add_scores_operand", "operand");
  p = Valid(false); p.keys = 1025; Expect(p, "keys above 1024", "keys");
  p = Valid(false); p.pv.shift = 31; Expect(p, "multiplier / shift", "shift");
  // hostile values in every stride field: refused, and no signed overflow on the way
  const int64_t hostile[] = {INT64_MAX, INT64_MIN, INT32_MAX, (1LL << 31), -(1LL << 62)};
  for (int64_t h : hostile)
    for (int f = 0; f < 16; ++f) {
      p = Valid(true);
      p.batch[0] = p.batch[1] = 65535; p.rows = INT32_MAX; p.keys = 1024;
      int64_t* fields[16] = {&p.q_bstride[0], &p.q_bstride[1], &p.k_bstride[0], &p.k_bstride[1], &p.v_bstride[0],
                             &p.v_bstride[1], &p.out_bstride[0], &p.out_bstride[1], &p.q_row_stride, &p.k_row_stride,
                             &p.v_row_stride, &p.out_row_stride, &p.bias_bstride[0], &p.bias_bstride[1],
                             &p.bias_row_stride, &p.bias_key_stride};
      *fields[f] = h;
      if (!bh_attention_why(&p)) {
        std::printf("hostile %lld in field %d accepted\n", static_cast<long long>(h), f);
        ++g_failed;
      }
    }
  if (g_failed) return 1;
  std::printf("attn check ok\n");
  return 0;
}
