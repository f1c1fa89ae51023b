// Helpers shared by the HipModelExecutor translation units (model_executor.cc,
// lower.cc, fusion.cc, fusion_transformer.cc, job_batch.cc): small accessors and the float32 op set.
// The per-family Args functions are in lower_args.h, the launch record in launch.h.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "backend/hip/lower_args.h"
#include "backend/hip/model_executor.h"
#include "backend/hip/quant.h"

#define RETURN_STATUS_IF(expr)      \
  do {                              \
    absl::Status _st = (expr);      \
    if (!_st.ok()) return _st;      \
  } while (0)

namespace band {
namespace hip {
namespace ex {

// set while PrepareJobBatches constructs a variant executor: a kCPU variant
// then makes no host pool of its own (job_batch.cc)
extern thread_local bool t_variant_ctor;

// *ls without the launches a fusion pass marked dead (fusion.cc)
void DropDead(std::vector<Launch>* ls, const std::vector<bool>& dead);

constexpr size_t kAlign = 256;

inline std::string Hex(uint64_t v) {
  char b[32];
  std::snprintf(b, sizeof(b), "%llx", static_cast<unsigned long long>(v));
  return b;
}

inline absl::Status HipErr(int rc, const char* what) {
  return absl::InternalError(std::string("HIP Error: ") + what + " (" + std::to_string(rc) + "): " + bh_last_error());
}


// "<conv kernel>+add": a conv launch with the following ADD in its epilogue
inline const char* WithAdd(const char* k) {
  static const char* const names[][2] = {{"conv_mfma_kernel", "conv_mfma_kernel+add"},
                                         {"conv_xs_kernel", "conv_xs_kernel+add"},
                                         {"conv_rows_kernel", "conv_rows_kernel+add"},
                                         {"conv_direct_kernel", "conv_direct_kernel+add"},
                                         {"conv_stem_kernel", "conv_stem_kernel+add"},
                                         {"conv_grouped_mfma_kernel", "conv_grouped_mfma_kernel+add"},
                                         {"conv_grouped_host", "conv_grouped_host+add"}};
  for (const auto& n : names)
    if (std::strcmp(k, n[0]) == 0) return n[1];
  return k;
}

inline int64_t MaxAbs(const int32_t* v, int n) {
  int64_t m = 0;
  for (int i = 0; v && i < n; ++i) m = std::max<int64_t>(m, v[i] < 0 ? -(int64_t)v[i] : (int64_t)v[i]);
  return m;
}

inline float HalfToFloat(uint16_t h) {
  const uint32_t sign = (h & 0x8000u) << 16;
  uint32_t exp = (h >> 10) & 0x1fu, man = h & 0x3ffu, bits;
  if (exp == 0) {
    if (man == 0) {
      bits = sign;
    } else {  // subnormal: renormalise
      exp = 127 - 15 + 1;
      while (!(man & 0x400u)) {
        man <<= 1;
        --exp;
      }
      bits = sign | (exp << 23) | ((man & 0x3ffu) << 13);
    }
  } else if (exp == 31) {
    bits = sign | 0x7f800000u | (man << 13);
  } else {
    bits = sign | ((exp + 127 - 15) << 23) | (man << 13);
  }
  float f;
  std::memcpy(&f, &bits, 4);
  return f;
}
// float values of a ConstFloat tensor
inline std::vector<float> FloatData(const TflModel& m, int t) {
  const TflTensor* src = &m.tensors[t];
  if (!src->is_const()) src = &m.tensors[ProducerOf(m, t)->inputs[0]];
  const size_t n = src->num_elements();
  std::vector<float> v(n);
  if (src->type == DataType::kFloat32) {
    std::memcpy(v.data(), src->data, 4 * n);
  } else {
    for (size_t i = 0; i < n; ++i) {
      uint16_t h;
      std::memcpy(&h, src->data + 2 * i, 2);
      v[i] = HalfToFloat(h);
    }
  }
  return v;
}
// fused activation bounds of a float op (kernels/kernel_util.h
// CalculateActivationRange)
inline void FloatActRange(int act, float* lo, float* hi) {
  const float inf = std::numeric_limits<float>::infinity();
  *lo = act == 1 || act == 3 ? 0.f : (act == 2 ? -1.f : -inf);
  *hi = act == 3 ? 6.f : (act == 2 ? 1.f : inf);
}

inline bool IsFloatOp(const TflModel& m, const TflOperator& op) {
  if (op.inputs.empty() || op.inputs[0] < 0) return false;
  const DataType t = m.tensors[op.inputs[0]].type;
  switch (op.builtin) {
    case kTflBatchMatMul:
    case kTflConv2D: case kTflDepthwiseConv2D: case kTflFullyConnected: case kTflAdd: case kTflSub: case kTflMul:
    case kTflAveragePool2D: case kTflMaxPool2D: case kTflRelu: case kTflRelu6: case kTflReluN1To1:
    case kTflLogistic: case kTflSoftmax: case kTflSquaredDifference: case kTflRsqrt: case kTflGelu: case kTflTanh:
      return t == DataType::kFloat32;
    case kTflDequantize:
      return t == DataType::kFloat16;
    default:
      return false;
  }
}
// the float32 op set (fp16-weight models)
// hybrid_conv: the executor was built with BAND_HIP_HYBRID_CONV=1
inline bool FloatSupports(const TflModel& m, const TflOperator& op, std::string* why, bool hybrid_conv = false) {
  auto no = [&](const char* w) {
    if (why) *why = w;
    return false;
  };
  const TflTensor& in = m.tensors[op.inputs[0]];
  const TflTensor& out = m.tensors[op.outputs[0]];
  if (op.builtin == kTflDequantize)
    return in.is_const() && out.type == DataType::kFloat32 ? true : no("float16 DEQUANTIZE of a constant only");
  if (IsHybridWeightOp(m, op)) {
    const char* w = "";
    if (op.builtin != kTflFullyConnected) {
      if (!hybrid_conv) return no("hybrid CONV_2D / DEPTHWISE_CONV_2D (float32 input, int8 filter)");
      return HybridConvArgs(m, op, nullptr, &w) ? true : no(w);
    }
    return HybridFcArgs(m, op, nullptr, &w) ? true : no(w);
  }
  if (out.type != DataType::kFloat32) return no("float32 output expected");
  switch (op.builtin) {
    case kTflConv2D:
    case kTflDepthwiseConv2D:
    case kTflFullyConnected: {
      if (op.inputs.size() < 2 || !ConstFloat(m, op.inputs[1])) return no("filter must be a float constant");
      if (op.inputs.size() > 2 && op.inputs[2] >= 0 && !ConstFloat(m, op.inputs[2]))
        return no("bias must be a float constant");
      const char* w = "";
      const bool ok = op.builtin == kTflFullyConnected ? FcArgs(m, op, nullptr, &w) : ConvArgs(m, op, nullptr, &w);
      return ok ? true : no(w);
    }
    case kTflAdd:
    case kTflSub:
    case kTflMul:
    case kTflSquaredDifference: {
      const char* w = "";
      if (!BroadcastArgs(m, op, nullptr, &w)) return no(w);
      return m.tensors[op.inputs[1]].type == DataType::kFloat32 ? true : no("float32 operands expected");
    }
    case kTflAveragePool2D:
    case kTflMaxPool2D: {
      const char* w = "";
      return PoolArgs(m, op, nullptr, &w) ? true : no(w);
    }
    case kTflSoftmax:
      return !in.shape.empty() ? true : no("rank >= 1");
    case kTflBatchMatMul: {
      const char* w = "";
      return BatchMatMulArgs(m, op, nullptr, &w) ? true : no(w);
    }
    case kTflTanh: {
      const char* w = "";
      return TanhArgs(m, op, nullptr, &w) ? true : no(w);
    }
    default:
      return true;  // RELU / RELU6 / RELU_N1_TO_1 / LOGISTIC / RSQRT / GELU
  }
}

}  // namespace ex
}  // namespace hip
}  // namespace band
