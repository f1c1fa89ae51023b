// The residual ADD folded into an int8 layer's epilogue: the device
// restatement of TFLite 2.9.2's add.cc / reference_integer_ops::Add for two
// 8-bit operands, y (the layer's own requantised value) and r (the residual
// byte).  Each operand is rescaled on its own,
//   s = MultiplyByQuantizedMultiplierSmallerThanOneExp((q + off) << left_shift, mult, shift)
// and the sum is requantised, offset and clamped.  Every kernel that folds
// the ADD states it through this header; the constructors below are the only
// places that name the parameter blocks' add fields.
#pragma once

#include "common.hpp"

namespace bh {

struct ResidualAdd {
  int32_t y_off, r_off, o_off;  // negated zero points of y / r, output zero point
  int32_t left_shift;
  int32_t y_mult, y_shift, r_mult, r_shift, o_mult, o_shift;
  int32_t act_min, act_max;
};

__device__ __forceinline__ ResidualAdd residual_of(const bh_conv_params& p) {
  return {p.add_y_off,  p.add_r_off,   p.add_o_off,  p.add_left_shift, p.add_y_mult,  p.add_y_shift,
          p.add_r_mult, p.add_r_shift, p.add_o_mult, p.add_o_shift,    p.add_act_min, p.add_act_max};
}
// the inverted-residual block: y is the projection's output p, r the block input x
__device__ __forceinline__ ResidualAdd residual_of(const bh_irb_params& p) {
  return {p.add_p_off,  p.add_x_off,   p.add_o_off,  p.add_left_shift, p.add_p_mult,  p.add_p_shift,
          p.add_x_mult, p.add_x_shift, p.add_o_mult, p.add_o_shift,    p.add_act_min, p.add_act_max};
}
// the attention core's masked form: y is the score, r the bias byte; the block names the ADD's operands a and
// b in the order the op lists them, and scores_operand says which of the two the scores are
__device__ __forceinline__ ResidualAdd residual_of(const bh_attention_add& p, int scores_operand) {
  if (scores_operand == 0)
    return {p.a_off,  p.b_off,   p.o_off,  p.left_shift, p.a_mult,  p.a_shift,
            p.b_mult, p.b_shift, p.o_mult, p.o_shift,    p.act_min, p.act_max};
  return {p.b_off,  p.a_off,   p.o_off,  p.left_shift, p.b_mult,  p.b_shift,
          p.a_mult, p.a_shift, p.o_mult, p.o_shift,    p.act_min, p.act_max};
}

// the rescaling of y / of r
__device__ __forceinline__ int32_t residual_scale_y(const ResidualAdd& A, int32_t v) {
  return requant_lt1((v + A.y_off) * (1 << A.left_shift), A.y_mult, A.y_shift);
}
__device__ __forceinline__ int32_t residual_scale_r(const ResidualAdd& A, int32_t q) {
  return requant_lt1((q + A.r_off) * (1 << A.left_shift), A.r_mult, A.r_shift);
}
// the rescaled operands' sum -> the output value
__device__ __forceinline__ int32_t residual_sum(const ResidualAdd& A, int32_t sy, int32_t sr) {
  return clamp_i32(requant_lt1(sy + sr, A.o_mult, A.o_shift) + A.o_off, A.act_min, A.act_max);
}

// Direct form: ADD(v, q) for the layer's value v and the residual value q.
__device__ __forceinline__ int32_t residual_add(const ResidualAdd& A, int32_t v, int32_t q) {
  return residual_sum(A, residual_scale_y(A, v), residual_scale_r(A, q));
}

// Table form, for int8 operands: both rescalings as 256-entry tables in LDS,
// tab[0, 256) for y and tab[256, 512) for r, indexed by value + 128.  Thread
// `tid` of `nthreads` builds its share; the caller places the barrier
// between the build and the first residual_add_tab.  Both rescalings of an
// entry are computed and one is kept: written as a choice between the two
// calls, the compiler chooses between their constants instead and serialises
// the arithmetic of a thread's entries (profiles/r19a_epilogue_bench.txt).
__device__ __forceinline__ void residual_tab_build(int* tab, const bh_conv_params& p, int tid, int nthreads) {
  for (int i = tid; i < 512; i += nthreads) {
    const int q = (i & 255) - 128;
    const int32_t sy = residual_scale_y(residual_of(p), q), sr = residual_scale_r(residual_of(p), q);
    tab[i] = i < 256 ? sy : sr;
  }
}
__device__ __forceinline__ int32_t residual_add_tab(const int* tab, const ResidualAdd& A, int32_t v, int32_t rq) {
  return residual_sum(A, tab[v + 128], tab[256 + rq + 128]);
}

// byte r of a residual dword as a value of the activation type
__device__ __forceinline__ int32_t residual_byte(uint32_t rq, int r, bool is_signed) {
  const uint32_t qb = (rq >> (8 * r)) & 0xffu;
  return is_signed ? (int32_t)(int8_t)qb : (int32_t)qb;
}

}  // namespace bh
