/* bh_attention_i8's parameter check: pure host code, shared by the launcher
 * (attention.hip) and the stand-alone sanitizer program of
 * tests/native/attn_check_test.cc. */
#pragma once

#include <limits.h>

#include <initializer_list>
#include <stdint.h>

#include "band_hip_kernels.h"

#define BH_ATTENTION_ROWS 64 /* query rows per workgroup (kAttnRows) */

/* NULL = runnable, else the reason */
inline const char* bh_attention_why(const bh_attention_params* p) {
  if (!p) return "null parameter block";
  if (!p->q || !p->k || !p->v || !p->out || !p->table) return "null pointer";
  if (p->rows <= 0 || p->keys <= 0 || p->head_dim <= 0 || p->out_dim <= 0 || p->batch[0] <= 0 || p->batch[1] <= 0)
    return "non-positive extent";
  if (p->keys > BH_ATTENTION_MAX_KEYS) return "keys above 1024 (the LDS strip of the scores)";
  if (p->head_dim > BH_ATTENTION_MAX_DIM) return "head_dim above 128 (the q fragments a wave keeps)";
  if (p->out_dim > BH_ATTENTION_MAX_DIM) return "out_dim above 128 (eight accumulator tiles per wave)";
  if (p->batch[0] > 65535 || p->batch[1] > 65535) return "a batch dim above 65535 (grid y / z)";
  const int64_t* bs[4] = {p->q_bstride, p->k_bstride, p->v_bstride, p->out_bstride};
  const int64_t rstr[4] = {p->q_row_stride, p->k_row_stride, p->v_row_stride, p->out_row_stride};
  const int64_t istr[4] = {p->q_inner_stride, p->k_inner_stride, p->v_inner_stride, p->out_inner_stride};
  const int64_t nrow[4] = {p->rows, p->keys, p->keys, p->rows};
  const int64_t ncol[4] = {p->head_dim, p->head_dim, p->out_dim, p->out_dim};
  for (int i = 0; i < 4; ++i)
    if (bs[i][0] < 0 || bs[i][1] < 0 || rstr[i] < 0 || istr[i] < 0) return "negative stride";
  for (int i = 0; i < 4; ++i)
    if (istr[i] != 1) return "non-unit inner stride";
  /* (a stride of 2^31 or more can address nothing valid, and keeps the span sums below inside 64 bits) */
  for (int i = 0; i < 4; ++i)
    if (bs[i][0] > INT32_MAX || bs[i][1] > INT32_MAX || rstr[i] > INT32_MAX) return "a tensor of 2^31 or more elements";
  for (int i = 0; i < 4; ++i) {
    const long long span = (p->batch[0] - 1LL) * bs[i][0] + (p->batch[1] - 1LL) * bs[i][1] + (nrow[i] - 1LL) * rstr[i] +
                           (ncol[i] - 1LL);
    if (span >= INT32_MAX) return "a tensor of 2^31 or more elements";
  }
  if (((p->rows + BH_ATTENTION_ROWS - 1LL) / BH_ATTENTION_ROWS) > INT32_MAX) return "a tensor of 2^31 or more elements";
  for (const bh_attention_quant* z : {&p->qk, &p->pv})
    if (z->shift > 30 || z->shift < -31 || z->mult < 0) return "multiplier / shift out of range";
  if (!p->bias) return 0;
  // the masked form
  if (p->bias_bstride[0] < 0 || p->bias_bstride[1] < 0 || p->bias_row_stride < 0 || p->bias_key_stride < 0)
    return "negative bias stride";
  if (p->bias_key_stride > 1) return "a bias key stride other than 0 or 1";
  if (p->bias_bstride[0] > INT32_MAX || p->bias_bstride[1] > INT32_MAX || p->bias_row_stride > INT32_MAX)
    return "a bias of 2^31 or more elements";
  const long long bspan = (p->batch[0] - 1LL) * p->bias_bstride[0] + (p->batch[1] - 1LL) * p->bias_bstride[1] +
                          (p->rows - 1LL) * p->bias_row_stride + (p->keys - 1LL) * p->bias_key_stride;
  if (bspan >= INT32_MAX) return "a bias of 2^31 or more elements";
  const bh_attention_add& a = p->add;
  if (a.a_shift > 0 || a.b_shift > 0) return "an ADD input shift above 0";
  if (a.o_shift > 0 || a.a_shift < -31 || a.b_shift < -31 || a.o_shift < -31) return "an ADD shift outside -31 .. 0";
  if (a.left_shift < 0 || a.left_shift > 31) return "an ADD left_shift outside 0 .. 31";
  if (a.act_min > a.act_max) return "an ADD activation window with act_min > act_max";
  if (p->add_scores_operand != 0 && p->add_scores_operand != 1) return "add_scores_operand other than 0 or 1";
  return 0;
}
