#include "backend/hip/lower_args.h"

#include <algorithm>
#include <cstring>
#include <limits>
#include <set>

namespace band {
namespace hip {
namespace ex {

namespace {

// the buffer of a constant holds its shape's elements (the reader bounds the
// buffer, not the shape against it)
bool Holds(const TflTensor& t) { return t.data_size >= t.num_elements() * GetDataTypeBytes(t.type); }

// a constant operand as the packers read it: the tensor, or the float16
// constant behind its DEQUANTIZE
bool ConstHolds(const TflModel& m, int t) {
  const TflTensor* c = &m.tensors[t];
  if (!c->is_const() && FoldableF16(m, t)) c = &m.tensors[ProducerOf(m, t)->inputs[0]];
  return !c->is_const() || Holds(*c);
}

bool Positive(const std::vector<int>& shape) {
  return std::all_of(shape.begin(), shape.end(), [](int d) { return d >= 1; });
}

}  // namespace

const TflOperator* ProducerOf(const TflModel& m, int t) {
  for (const TflOperator& op : m.ops)
    for (int o : op.outputs)
      if (o == t) return &op;
  return nullptr;
}

bool FoldableF16(const TflModel& m, int t) {
  if (t < 0 || m.tensors[t].type != DataType::kFloat32) return false;
  const TflOperator* p = ProducerOf(m, t);
  return p && p->builtin == kTflDequantize && !p->inputs.empty() && p->inputs[0] >= 0 &&
         m.tensors[p->inputs[0]].is_const() && m.tensors[p->inputs[0]].type == DataType::kFloat16;
}

bool ConvArgs(const TflModel& m, const TflOperator& op, ConvGeometry* g, const char** why) {
  auto no = [&](const char* w) {
    if (why) *why = w;
    return false;
  };
  const bool dw = op.builtin == kTflDepthwiseConv2D, tc = op.builtin == kTflTransposeConv;
  if (op.builtin != kTflConv2D && !dw && !tc) return no("not a convolution");
  // TRANSPOSE_CONV inputs: output_shape (const int32 [4]), filter OHWI, input, [bias]
  const size_t xi = tc ? 2 : 0, bi = tc ? 3 : 2;
  if (op.inputs.size() <= std::max<size_t>(xi, 1) || op.inputs[xi] < 0 || op.inputs[1] < 0 || op.outputs.empty() ||
      op.outputs[0] < 0)
    return no("missing operands");
  ConvGeometry c{};
  c.input = op.inputs[xi];
  c.filter = op.inputs[1];
  c.bias = op.inputs.size() > bi ? op.inputs[bi] : -1;
  const TflTensor& in = m.tensors[c.input];
  const TflTensor& w = m.tensors[c.filter];
  const TflTensor& out = m.tensors[op.outputs[0]];
  if (in.shape.size() != 4 || w.shape.size() != 4 || out.shape.size() != 4)
    return no(tc ? "4-D, filter [oc][kh][kw][ic]" : "conv needs 4-D");
  if (!Positive(w.shape)) return no("filter dims must be >= 1");
  if (!Positive(in.shape)) return no("empty input");
  c.batch = in.shape[0]; c.in_h = in.shape[1]; c.in_w = in.shape[2]; c.in_c = in.shape[3];
  c.out_c = dw ? w.shape[3] : w.shape[0];
  c.k_h = w.shape[1]; c.k_w = w.shape[2];
  c.groups = c.depth_multiplier = 1;
  if (tc && w.shape[3] != c.in_c) return no("4-D, filter [oc][kh][kw][ic]");
  if (op.builtin == kTflConv2D && w.shape[3] != c.in_c) {
    // grouped: groups = in_c / filter_in_c must divide both channel counts
    if (in.type == DataType::kFloat32) return no("grouped conv: int8 / uint8 only");
    if (c.in_c % w.shape[3] != 0) return no("grouped conv: input channels not a multiple of the filter's");
    c.groups = c.in_c / w.shape[3];
    if (c.out_c % c.groups != 0) return no("grouped conv: output channels not a multiple of the group count");
  }
  if (dw) {
    if (c.out_c % c.in_c != 0) return no("bad depth multiplier");
    c.depth_multiplier = c.out_c / c.in_c;
  }
  // Conv2DOptions: padding, stride_w, stride_h, activation, dilation_w, dilation_h;
  // DepthwiseConv2DOptions has depth_multiplier at slot 3; TransposeConvOptions
  // has the first three only (an absent table reads as the defaults)
  const FbTable& o = op.options;
  const bool same = o.Int8(0, 0) == 0;
  c.stride_w = o.Int(1, 1); c.stride_h = o.Int(2, 1);
  c.act = tc ? 0 : o.Int8(dw ? 4 : 3, 0);
  c.dil_w = tc ? 1 : o.Int(dw ? 5 : 4, 1);
  c.dil_h = tc ? 1 : o.Int(dw ? 6 : 5, 1);
  if (c.stride_h < 1 || c.stride_w < 1) return no("strides must be >= 1");
  if (c.dil_h < 1 || c.dil_w < 1) return no("dilations must be >= 1");
  if (tc) {
    // transpose_conv.cc: the output is the input of the forward conv
    c.out_h = out.shape[1]; c.out_w = out.shape[2];
    if (out.shape[0] != c.batch || out.shape[3] != c.out_c || c.out_h < 1 || c.out_w < 1 ||
        ComputeOutSize(same, c.out_h, c.k_h, c.stride_h, 1) != c.in_h ||
        ComputeOutSize(same, c.out_w, c.k_w, c.stride_w, 1) != c.in_w)
      return no("TRANSPOSE_CONV shape mismatch");
    c.pad_h = ComputePadding(c.stride_h, 1, c.out_h, c.k_h, c.in_h);
    c.pad_w = ComputePadding(c.stride_w, 1, c.out_w, c.k_w, c.in_w);
  } else {
    c.out_h = ComputeOutSize(same, c.in_h, c.k_h, c.stride_h, c.dil_h);
    c.out_w = ComputeOutSize(same, c.in_w, c.k_w, c.stride_w, c.dil_w);
    if (out.shape != std::vector<int>{c.batch, c.out_h, c.out_w, c.out_c}) return no("conv output shape mismatch");
    if (c.out_h < 1 || c.out_w < 1) return no("empty output");
    c.pad_h = ComputePadding(c.stride_h, c.dil_h, c.in_h, c.k_h, c.out_h);
    c.pad_w = ComputePadding(c.stride_w, c.dil_w, c.in_w, c.k_w, c.out_w);
  }
  if (!ConstHolds(m, c.filter)) return no("filter data smaller than its shape");
  if (c.bias >= 0) {
    if (m.tensors[c.bias].num_elements() != static_cast<size_t>(c.out_c))
      return no("bias element count differs from the output channels");
    if (!ConstHolds(m, c.bias)) return no("bias data smaller than its shape");
  }
  if (IsQ8(in.type) && w.scale.size() != 1 && w.scale.size() != static_cast<size_t>(c.out_c))
    return no("filter scale count is neither 1 nor the output channels");
  if (g) *g = c;
  return true;
}

bool FcArgs(const TflModel& m, const TflOperator& op, FcGeometry* g, const char** why) {
  auto no = [&](const char* w) {
    if (why) *why = w;
    return false;
  };
  if (op.builtin != kTflFullyConnected || op.inputs.size() < 2 || op.inputs[0] < 0 || op.inputs[1] < 0 ||
      op.outputs.empty() || op.outputs[0] < 0)
    return no("missing operands");
  FcGeometry f{};
  f.filter = op.inputs[1];
  f.bias = op.inputs.size() > 2 ? op.inputs[2] : -1;
  const TflTensor& in = m.tensors[op.inputs[0]];
  const TflTensor& w = m.tensors[f.filter];
  if (w.shape.size() != 2) return no("FC weights must be 2-D");
  f.units = w.shape[0];
  f.depth = w.shape[1];
  if (f.depth < 1) return no("FULLY_CONNECTED depth must be >= 1");
  if (f.units < 1) return no("FULLY_CONNECTED units must be >= 1");
  if (in.num_elements() == 0 || in.num_elements() % static_cast<size_t>(f.depth) != 0)
    return no("FC input/depth mismatch");
  if (in.num_elements() / f.depth > 0x7fffffffu) return no("FC input of 2^31 or more rows");
  f.rows = static_cast<int>(in.num_elements() / f.depth);
  f.act = op.options.Int8(0, 0);
  if (!ConstHolds(m, f.filter)) return no("filter data smaller than its shape");
  if (f.bias >= 0) {
    if (m.tensors[f.bias].num_elements() != static_cast<size_t>(f.units))
      return no("bias element count differs from the units");
    if (!ConstHolds(m, f.bias)) return no("bias data smaller than its shape");
  }
  if (m.tensors[op.outputs[0]].num_elements() != static_cast<size_t>(f.rows) * f.units)
    return no("FC output shape mismatch");
  if (g) *g = f;
  return true;
}

bool HybridFcArgs(const TflModel& m, const TflOperator& op, HybridFcGeometry* g, const char** why) {
  auto no = [&](const char* w) {
    if (why) *why = w;
    return false;
  };
  if (op.builtin != kTflFullyConnected || !IsHybridWeightOp(m, op) || op.outputs.empty() || op.outputs[0] < 0)
    return no("not a hybrid FULLY_CONNECTED");
  const TflTensor& w = m.tensors[op.inputs[1]];
  if (w.type != DataType::kInt8) return no("hybrid FULLY_CONNECTED: uint8 filter (int8 only)");
  if (!w.is_const()) return no("hybrid FULLY_CONNECTED: filter must be a constant");
  if (w.scale.size() > 1) return no("hybrid FULLY_CONNECTED: per-channel filter scales");
  if (w.scale.size() != 1 || !(w.scale[0] > 0.f)) return no("hybrid FULLY_CONNECTED: filter needs one positive scale");
  if (Zp(w) != 0 || w.zero_point.size() > 1) return no("hybrid FULLY_CONNECTED: non-zero filter zero point");
  // FullyConnectedOptions: fused activation, weights_format, keep_num_dims, asymmetric_quantize_inputs
  if (op.options.Int8(1, 0) != 0) return no("hybrid FULLY_CONNECTED: weights_format != 0");
  if (op.inputs.size() > 2 && op.inputs[2] >= 0 && !ConstFloat(m, op.inputs[2]))
    return no("hybrid FULLY_CONNECTED: bias must be a float constant");
  if (m.tensors[op.outputs[0]].type != DataType::kFloat32) return no("hybrid FULLY_CONNECTED: float32 output expected");
  HybridFcGeometry h{};
  const char* r = "";
  if (!FcArgs(m, op, &h.fc, &r)) return no(r);
  if (h.fc.depth > 65535) return no("hybrid FULLY_CONNECTED: depth > 65,535 (the int32 dot)");
  if (static_cast<long long>(h.fc.rows) * h.fc.depth > 0x7fffffffLL ||
      static_cast<long long>(h.fc.rows) * h.fc.units > 0x7fffffffLL ||
      static_cast<long long>(h.fc.units) * ((h.fc.depth + 15) / 16 * 16) > 0x7fffffffLL)
    return no("hybrid FULLY_CONNECTED: a tensor of 2^31 or more elements");
  h.w_scale = w.scale[0];
  h.asymmetric = op.options.valid() && op.options.Bool(3, false);
  if (g) *g = h;
  return true;
}

bool HybridConvArgs(const TflModel& m, const TflOperator& op, HybridConvGeometry* g, const char** why) {
  auto no = [&](const char* w) {
    if (why) *why = w;
    return false;
  };
  if (!IsHybridConvOp(m, op) || op.outputs.empty() || op.outputs[0] < 0) return no("not a hybrid CONV_2D / DEPTHWISE_CONV_2D");
  const bool dw = op.builtin == kTflDepthwiseConv2D;
  // one literal per op and reason: `why` outlives the call
#define BH_HY(reason) (dw ? "hybrid DEPTHWISE_CONV_2D: " reason : "hybrid CONV_2D: " reason)
  const TflTensor& in = m.tensors[op.inputs[0]];
  const TflTensor& w = m.tensors[op.inputs[1]];
  if (w.type != DataType::kInt8) return no(BH_HY("uint8 filter (int8 only)"));
  if (!w.is_const()) return no(BH_HY("filter must be a constant"));
  if (op.inputs.size() > 2 && op.inputs[2] >= 0) {
    const TflTensor& b = m.tensors[op.inputs[2]];
    if (!b.is_const() || b.type != DataType::kFloat32) return no(BH_HY("bias must be a float32 constant"));
  }
  if (m.tensors[op.outputs[0]].type != DataType::kFloat32) return no(BH_HY("float32 output expected"));
  for (int64_t z : w.zero_point)
    if (z != 0) return no(BH_HY("non-zero filter zero point"));
  if (!dw && in.shape.size() == 4 && w.shape.size() == 4 && w.shape[3] != in.shape[3])
    return no(BH_HY("grouped filter (in_c / G input channels)"));
  HybridConvGeometry h{};
  const char* r = "";
  if (!ConvArgs(m, op, &h.conv, &r)) return no(r);
  const ConvGeometry& c = h.conv;
  const size_t ns = w.scale.size();
  if (ns != 1 && ns != static_cast<size_t>(c.out_c)) return no(BH_HY("filter scale count is neither 1 nor the output channels"));
  for (float s : w.scale)
    if (!(s > 0.f)) return no(BH_HY("filter scales must be positive"));
  h.depthwise = dw;
  h.per_channel = dw || ns > 1;
  if (dw && ns == 1 && c.out_c != 1) return no(BH_HY("one filter scale (per-channel only)"));
  const long long K = static_cast<long long>(c.k_h) * c.k_w * (dw ? 1 : c.in_c);
  if (K > 65535) return no(BH_HY("k_h * k_w * in_c > 65,535 (the int32 sum)"));
  if (static_cast<long long>(c.batch) * c.in_h * c.in_w * c.in_c > 0x7fffffffLL ||
      static_cast<long long>(c.batch) * c.out_h * c.out_w * c.out_c > 0x7fffffffLL ||
      static_cast<long long>(c.out_c) * ((K + 15) / 16 * 16) > 0x7fffffffLL)
    return no(BH_HY("a tensor of 2^31 or more elements"));
#undef BH_HY
  h.w_scale.assign(c.out_c, w.scale[0]);
  if (ns > 1) h.w_scale = w.scale;
  if (g) *g = std::move(h);
  return true;
}

bool PoolArgs(const TflModel& m, const TflOperator& op, PoolGeometry* g, const char** why) {
  auto no = [&](const char* w) {
    if (why) *why = w;
    return false;
  };
  if ((op.builtin != kTflAveragePool2D && op.builtin != kTflMaxPool2D) || op.inputs.empty() || op.inputs[0] < 0 ||
      op.outputs.empty() || op.outputs[0] < 0)
    return no("missing operands");
  const TflTensor& in = m.tensors[op.inputs[0]];
  const TflTensor& out = m.tensors[op.outputs[0]];
  if (in.shape.size() != 4 || out.shape.size() != 4) return no("4-D only");
  if (!Positive(in.shape)) return no("empty input");
  // Pool2DOptions: padding, stride_w, stride_h, filter_width, filter_height, activation
  const FbTable& o = op.options;
  const bool same = o.Int8(0, 0) == 0;
  PoolGeometry p{};
  p.batch = in.shape[0]; p.in_h = in.shape[1]; p.in_w = in.shape[2]; p.channels = in.shape[3];
  p.stride_w = o.Int(1, 1); p.stride_h = o.Int(2, 1); p.f_w = o.Int(3, 1); p.f_h = o.Int(4, 1);
  p.act = o.Int8(5, 0);
  if (p.stride_h < 1 || p.stride_w < 1) return no("strides must be >= 1");
  if (p.f_h < 1 || p.f_w < 1) return no("pool filter must be >= 1");
  p.out_h = ComputeOutSize(same, p.in_h, p.f_h, p.stride_h, 1);
  p.out_w = ComputeOutSize(same, p.in_w, p.f_w, p.stride_w, 1);
  if (out.shape != std::vector<int>{p.batch, p.out_h, p.out_w, p.channels}) return no("pool output shape mismatch");
  if (p.out_h < 1 || p.out_w < 1) return no("empty output");
  p.pad_h = ComputePadding(p.stride_h, 1, p.in_h, p.f_h, p.out_h);
  p.pad_w = ComputePadding(p.stride_w, 1, p.in_w, p.f_w, p.out_w);
  if (g) *g = p;
  return true;
}

bool BroadcastArgs(const TflModel& m, const TflOperator& op, BroadcastShapes* s, const char** why) {
  auto no = [&](const char* w) {
    if (why) *why = w;
    return false;
  };
  if (op.inputs.size() != 2 || op.inputs[0] < 0 || op.inputs[1] < 0 || op.outputs.empty() || op.outputs[0] < 0)
    return no("binary op needs 2 inputs");
  const TflTensor& a = m.tensors[op.inputs[0]];
  const TflTensor& b = m.tensors[op.inputs[1]];
  const TflTensor& out = m.tensors[op.outputs[0]];
  if (a.shape.size() > 4 || b.shape.size() > 4 || out.shape.size() > 4) return no("rank > 4");
  BroadcastShapes r;
  Shape4(a.shape, r.a);
  Shape4(b.shape, r.b);
  Shape4(out.shape, r.o);
  for (int d = 0; d < 4; ++d)
    if ((r.a[d] != r.o[d] && r.a[d] != 1) || (r.b[d] != r.o[d] && r.b[d] != 1)) return no("bad broadcast");
  if (!ConstHolds(m, op.inputs[0]) || !ConstHolds(m, op.inputs[1])) return no("constant data smaller than its shape");
  if (s) *s = r;
  return true;
}

bool BatchMatMulArgs(const TflModel& m, const TflOperator& op, bh_batch_matmul_params* p,
                     const char** why, bool* batch_axis_ok) {
  auto no = [&](const char* w) {
    if (why) *why = w;
    return false;
  };
  if (op.builtin != kTflBatchMatMul || op.inputs.size() < 2 || op.inputs[0] < 0 || op.inputs[1] < 0 ||
      op.outputs.empty() || op.outputs[0] < 0)
    return no("missing operands");
  const TflTensor& l = m.tensors[op.inputs[0]];
  const TflTensor& r = m.tensors[op.inputs[1]];
  const TflTensor& o = m.tensors[op.outputs[0]];
  if (l.type == DataType::kFloat32 && r.type == DataType::kInt8)
    return no("hybrid BATCH_MATMUL (float32 lhs, int8 rhs)");
  if (l.type != r.type || l.type != o.type) return no("BATCH_MATMUL operands and output differ in type");
  if (l.type != DataType::kInt8 && l.type != DataType::kFloat32)
    return no("BATCH_MATMUL: int8 and float32 only (no uint8, no int16)");
  const bool i8 = l.type == DataType::kInt8;
  if (i8 && (!HasQ(l) || !HasQ(r) || !HasQ(o))) return no("missing quantization");
  const int rl = static_cast<int>(l.shape.size()), rr = static_cast<int>(r.shape.size());
  const int ro = static_cast<int>(o.shape.size());
  if (rl < 2 || rr < 2 || rl > 4 || rr > 4) return no("BATCH_MATMUL operands must have rank 2 to 4");
  if (ro != std::max(rl, rr)) return no("BATCH_MATMUL output rank differs from the operands' larger rank");
  const bool adj_x = op.options.valid() && op.options.Int8(0, 0) != 0;
  const bool adj_y = op.options.valid() && op.options.Int8(1, 0) != 0;
  const int64_t la = l.shape[rl - 2], lb = l.shape[rl - 1], ra = r.shape[rr - 2], rb = r.shape[rr - 1];
  const int64_t M = adj_x ? lb : la, K = adj_x ? la : lb;
  const int64_t Kr = adj_y ? rb : ra, N = adj_y ? ra : rb;
  if (M <= 0 || N <= 0 || K <= 0) return no("empty matrix");
  if (K != Kr) return no("BATCH_MATMUL: mismatched K");
  if (i8 && K > 32767) return no("BATCH_MATMUL: K > 32767");
  int64_t bl[2] = {1, 1}, br[2] = {1, 1}, bo[2] = {1, 1};
  for (int d = 0; d < rl - 2; ++d) bl[2 - (rl - 2) + d] = l.shape[d];
  for (int d = 0; d < rr - 2; ++d) br[2 - (rr - 2) + d] = r.shape[d];
  for (int d = 0; d < ro - 2; ++d) bo[2 - (ro - 2) + d] = o.shape[d];
  for (int d = 0; d < 2; ++d) {
    const int64_t want = std::max(bl[d], br[d]);
    if ((bl[d] != want && bl[d] != 1) || (br[d] != want && br[d] != 1))
      return no("BATCH_MATMUL: batch dims neither equal nor 1");
    if (bo[d] != want || want <= 0) return no("BATCH_MATMUL output shape mismatch");
  }
  if (o.shape[ro - 2] != M || o.shape[ro - 1] != N) return no("BATCH_MATMUL output shape mismatch");
  // the launchers' limits (bh_batch_matmul_check), so that a refusal surfaces here and not at prepare time
  if (bo[0] > 65535 || bo[1] > 65535) return no("BATCH_MATMUL: a batch dim above 65535");
  if (l.num_elements() > 0x7fffffffu || r.num_elements() > 0x7fffffffu || o.num_elements() > 0x7fffffffu)
    return no("BATCH_MATMUL: a tensor of 2^31 or more elements");
  if (p) {
    *p = bh_batch_matmul_params{};
    p->batch[0] = static_cast<int32_t>(bo[0]);
    p->batch[1] = static_cast<int32_t>(bo[1]);
    p->m = static_cast<int32_t>(M);
    p->n = static_cast<int32_t>(N);
    p->k = static_cast<int32_t>(K);
    p->lhs_bstride[1] = bl[1] == 1 ? 0 : la * lb;
    p->lhs_bstride[0] = bl[0] == 1 ? 0 : bl[1] * la * lb;
    p->rhs_bstride[1] = br[1] == 1 ? 0 : ra * rb;
    p->rhs_bstride[0] = br[0] == 1 ? 0 : br[1] * ra * rb;
    p->lhs_row_stride = adj_x ? 1 : lb;
    p->lhs_k_stride = adj_x ? lb : 1;
    p->rhs_k_stride = adj_y ? 1 : rb;
    p->rhs_col_stride = adj_y ? rb : 1;
    p->requant_fast = -1;  // the launcher decides
    if (i8) {
      p->lhs_zp = Zp(l);
      p->rhs_zp = Zp(r);
      p->out_zp = Zp(o);
      FullyConnectedMultiplier(Scale(l), Scale(r), Scale(o), &p->mult, &p->shift);
    }
  }
  if (batch_axis_ok) {
    auto rides = [&](const TflTensor& t, int rank) {
      if (t.is_const()) return rank < ro || t.shape[0] == 1;
      return rank == ro;
    };
    *batch_axis_ok = ro >= 3 && rides(l, rl) && rides(r, rr);
  }
  return true;
}

bool MirrorPadArgs(const TflModel& m, const TflOperator& op, std::vector<int64_t>* pads, int* mode) {
  if (op.inputs.size() < 2 || op.inputs[1] < 0) return false;
  const TflTensor& in = m.tensors[op.inputs[0]];
  const TflTensor& pt = m.tensors[op.inputs[1]];
  if (!pt.is_const() || (pt.type != DataType::kInt32 && pt.type != DataType::kInt64)) return false;
  const int rank = static_cast<int>(in.shape.size());
  const size_t eb = pt.type == DataType::kInt64 ? 8 : 4;
  if (rank < 1 || rank > 4 || pt.data_size < 2 * rank * eb) return false;
  pads->assign(2 * static_cast<size_t>(rank), 0);
  for (int i = 0; i < 2 * rank; ++i) {
    if (eb == 8) {
      int64_t v;
      std::memcpy(&v, pt.data + 8 * i, 8);
      (*pads)[i] = v;
    } else {
      int32_t v;
      std::memcpy(&v, pt.data + 4 * i, 4);
      (*pads)[i] = v;
    }
  }
  *mode = op.options.valid() && op.options.Int8(0, 0) == 1 ? 2 : 1;
  for (int dd = 0; dd < rank; ++dd) {
    const int64_t lim = in.shape[dd] - (*mode == 1 ? 1 : 0);
    if ((*pads)[2 * dd] < 0 || (*pads)[2 * dd + 1] < 0 || (*pads)[2 * dd] > lim || (*pads)[2 * dd + 1] > lim)
      return false;
  }
  return true;
}

bool MeanArgs(const TflModel& m, const TflOperator& op, MeanGeometry* g, const char** why) {
  auto no = [&](const char* w) {
    if (why) *why = w;
    return false;
  };
  if (op.builtin != kTflMean || op.inputs.size() < 2 || op.inputs[0] < 0 || op.inputs[1] < 0 || op.outputs.empty() ||
      op.outputs[0] < 0)
    return no("MEAN needs an input, an axes tensor and an output");
  const TflTensor& in = m.tensors[op.inputs[0]];
  const TflTensor& out = m.tensors[op.outputs[0]];
  const TflTensor& ax = m.tensors[op.inputs[1]];
  if (!ax.is_const() || ax.type != DataType::kInt32) return no("MEAN axes must be a constant int32 tensor");
  if (out.type != in.type) return no("MEAN output type differs from the input's");
  const int rank = static_cast<int>(in.shape.size());
  std::set<int> axes;
  for (size_t i = 0; i * 4 < ax.data_size; ++i) {
    int32_t v;
    std::memcpy(&v, ax.data + 4 * i, 4);
    if (v < 0) v += rank;
    if (v < 0 || v >= rank) return no("MEAN axis out of range");
    axes.insert(v);
  }
  if (axes.empty() || *axes.rbegin() - *axes.begin() + 1 != static_cast<int>(axes.size()))
    return no("MEAN over one contiguous run of axes only");
  MeanGeometry r{};
  if (in.type != DataType::kFloat32) {
    const bool keep = op.options.valid() && op.options.Int8(0, 0) != 0;
    if (!IsQ8(in.type)) return no("MEAN: int8, uint8 and float32 only");
    if (!HasQ(in) || !HasQ(out)) return no("missing quantization");
    const bool hw = rank == 4 && keep && axes == std::set<int>{1, 2};
    r.rows = !hw && rank >= 1 && rank <= 4 && axes == std::set<int>{rank - 1};
    if (!hw && !r.rows)
      return no("8-bit MEAN: 4-D keep_dims over axes {1, 2}, or rank 1-4 over the last axis");
    r.exact = Scale(in) == Scale(out) && Zp(in) == Zp(out);
  }
  r.outer = r.reduce = r.inner = 1;
  for (int dd = 0; dd < rank; ++dd) {
    if (dd < *axes.begin()) r.outer *= in.shape[dd];
    else if (dd > *axes.rbegin()) r.inner *= in.shape[dd];
    else r.reduce *= in.shape[dd];
  }
  r.reduces_axis0 = *axes.begin() == 0;
  if (r.reduce <= 0 || r.outer <= 0 || r.inner <= 0) return no("MEAN of an empty tensor");
  if (out.num_elements() != static_cast<size_t>(r.outer * r.inner))
    return no("MEAN output must hold outer * inner elements");
  // bh_mean_rows_check's limits, so that a refusal surfaces here and not at prepare time
  if (r.rows && r.reduce * 255 >= (1l << 31)) return no("8-bit MEAN: a row of 2^31 / 255 or more elements");
  if (g) *g = r;
  return true;
}

bool MeanArgs(const TflModel& m, const TflOperator& op, long* outer, long* reduce, long* inner) {
  MeanGeometry g;
  if (!MeanArgs(m, op, &g)) return false;
  *outer = g.outer;
  *reduce = g.reduce;
  *inner = g.inner;
  return true;
}

bool SquaredDifferenceArgs(const TflModel& m, const TflOperator& op, BroadcastShapes* s, AddParams* q,
                           const char** why) {
  auto no = [&](const char* w) {
    if (why) *why = w;
    return false;
  };
  if (op.builtin != kTflSquaredDifference) return no("not a SQUARED_DIFFERENCE");
  if (!BroadcastArgs(m, op, s, why)) return false;
  const TflTensor& a = m.tensors[op.inputs[0]];
  const TflTensor& b = m.tensors[op.inputs[1]];
  const TflTensor& out = m.tensors[op.outputs[0]];
  if (a.type != DataType::kInt8 || b.type != DataType::kInt8 || out.type != DataType::kInt8)
    return no("SQUARED_DIFFERENCE: int8 and float32 only (no uint8, no int16)");
  if (!HasQ(a) || !HasQ(b) || !HasQ(out)) return no("missing quantization");
  AddParams p;
  if (!SquaredDifferenceParams(Scale(a), Scale(b), Scale(out), &p, why)) return false;
  if (q) *q = p;
  return true;
}

bool ArgMinMaxArgs(const TflModel& m, const TflOperator& op, long* outer, long* axis_len, long* inner,
                   int* out_bytes, int* axis_out, const char** why) {
  auto no = [&](const char* w) {
    if (why) *why = w;
    return false;
  };
  if ((op.builtin != kTflArgMax && op.builtin != kTflArgMin) || op.inputs.size() < 2 || op.inputs[0] < 0 ||
      op.inputs[1] < 0 || op.outputs.empty() || op.outputs[0] < 0)
    return no("ARG_MAX / ARG_MIN needs an input, an axis and an output");
  const TflTensor& in = m.tensors[op.inputs[0]];
  const TflTensor& ax = m.tensors[op.inputs[1]];
  const TflTensor& out = m.tensors[op.outputs[0]];
  if (in.type != DataType::kInt8 && in.type != DataType::kUInt8 && in.type != DataType::kFloat32)
    return no("ARG_MAX / ARG_MIN input must be int8, uint8 or float32");
  const int rank = static_cast<int>(in.shape.size());
  if (rank < 1 || rank > 4) return no("ARG_MAX / ARG_MIN input rank must be 1-4");
  if (!ax.is_const()) return no("ARG_MAX / ARG_MIN axis must be a constant");
  if ((ax.type != DataType::kInt32 && ax.type != DataType::kInt64) || ax.num_elements() != 1 ||
      ax.data_size < (ax.type == DataType::kInt64 ? 8u : 4u))
    return no("ARG_MAX / ARG_MIN axis must be one int32 / int64 value");
  int64_t axis = 0;
  if (ax.type == DataType::kInt64) {
    std::memcpy(&axis, ax.data, 8);
  } else {
    int32_t v;
    std::memcpy(&v, ax.data, 4);
    axis = v;
  }
  if (axis < 0) axis += rank;
  if (axis < 0 || axis >= rank) return no("ARG_MAX / ARG_MIN axis out of range");
  if (out.type != DataType::kInt32 && out.type != DataType::kInt64)
    return no("ARG_MAX / ARG_MIN output must be int32 or int64");
  const int want = op.options.valid() ? op.options.Int8(0, 0) : 0;  // TensorType (schema default 0 = float32)
  if (want != (out.type == DataType::kInt64 ? 4 : 2))
    return no("ARG_MAX / ARG_MIN output type differs from output_type");
  *outer = *inner = 1;
  for (int dd = 0; dd < axis; ++dd) *outer *= in.shape[dd];
  for (int dd = static_cast<int>(axis) + 1; dd < rank; ++dd) *inner *= in.shape[dd];
  *axis_len = in.shape[axis];
  *out_bytes = out.type == DataType::kInt64 ? 8 : 4;
  if (axis_out) *axis_out = static_cast<int>(axis);
  if (*axis_len <= 0 || *outer <= 0 || *inner <= 0 || out.num_elements() != static_cast<size_t>(*outer * *inner))
    return no("ARG_MAX / ARG_MIN output must hold outer * inner elements");
  return true;
}

bool ConstInts(const TflTensor& t, std::vector<int64_t>* v) {
  if (!t.is_const() || (t.type != DataType::kInt32 && t.type != DataType::kInt64)) return false;
  const size_t eb = t.type == DataType::kInt64 ? 8 : 4, n = t.num_elements();
  if (t.data_size < n * eb) return false;
  v->resize(n);
  for (size_t i = 0; i < n; ++i) {
    if (eb == 8) {
      std::memcpy(&(*v)[i], t.data + 8 * i, 8);
    } else {
      int32_t x;
      std::memcpy(&x, t.data + 4 * i, 4);
      (*v)[i] = x;
    }
  }
  return true;
}

bool ReindexArgs(const TflModel& m, const TflOperator& op, int oi, bh_reindex_params* map,
                 const char** why, bool* whole_batch) {
  auto no = [&](const char* w) {
    if (why) *why = w;
    return false;
  };
  const int b = op.builtin;
  const int xin = b == kTflSplit ? 1 : 0;
  const size_t need = b == kTflStridedSlice ? 4 : (b == kTflSlice || b == kTflSplitV) ? 3
                      : (b == kTflTranspose || b == kTflSplit || b == kTflTile)      ? 2
                                                                                     : 1;
  if (!IsReindexOp(b) || op.inputs.size() < need || oi < 0 || oi >= static_cast<int>(op.outputs.size()) ||
      op.outputs[oi] < 0)
    return no("missing operands");
  for (size_t i = 0; i < need; ++i)
    if (op.inputs[i] < 0) return no("missing operands");
  const TflTensor& in = m.tensors[op.inputs[xin]];
  const TflTensor& out = m.tensors[op.outputs[oi]];
  if (in.type != DataType::kInt8 && in.type != DataType::kUInt8 && in.type != DataType::kFloat32 &&
      in.type != DataType::kInt32)
    return no("element type must be int8, uint8, float32 or int32");
  if (out.type != in.type) return no("output type differs from the input's");
  if (in.scale != out.scale || in.zero_point != out.zero_point)
    return no("output quantization differs from the input's (the op copies bytes)");
  if (out.num_elements() == 0) return no("output has no elements");
  const int r = static_cast<int>(in.shape.size());
  if (r > BH_REINDEX_MAX_RANK) return no("rank > 6");
  std::vector<int64_t> istr(r, 1);
  for (int d = r - 2; d >= 0; --d) istr[d] = istr[d + 1] * in.shape[d + 1];
  std::vector<int64_t> ext, str, expect;  // the map's extents / strides, the output shape they mean
  int64_t off = 0;
  bool lead = false;  // map dim 0 walks input axis 0 from element 0 at stride 1
  auto ints = [&](int input, std::vector<int64_t>* v) { return ConstInts(m.tensors[op.inputs[input]], v); };
  if (b == kTflTranspose) {
    std::vector<int64_t> perm;
    if (!ints(1, &perm)) return no("TRANSPOSE perm must be a constant int32 / int64 tensor");
    if (r > 5) return no("TRANSPOSE rank > 5");
    std::vector<bool> seen(r, false);
    if (static_cast<int>(perm.size()) != r) return no("TRANSPOSE perm is not a permutation");
    for (int64_t p : perm) {
      if (p < 0 || p >= r || seen[p]) return no("TRANSPOSE perm is not a permutation");
      seen[p] = true;
      ext.push_back(in.shape[p]);
      str.push_back(istr[p]);
    }
    lead = r > 0 && perm[0] == 0;
    expect = ext;
  } else if (b == kTflSlice) {
    std::vector<int64_t> begin, size;
    if (!ints(1, &begin) || !ints(2, &size)) return no("SLICE begin / size must be constant int32 / int64 tensors");
    if (r > 5) return no("SLICE rank > 5");
    if (static_cast<int>(begin.size()) != r || static_cast<int>(size.size()) != r)
      return no("SLICE begin / size length differs from the rank");
    for (int d = 0; d < r; ++d) {
      const int64_t n = in.shape[d], s = size[d] == -1 ? n - begin[d] : size[d];
      if (begin[d] < 0 || begin[d] > n || s < 0 || begin[d] + s > n) return no("SLICE begin / size outside the input");
      ext.push_back(s);
      str.push_back(istr[d]);
      off += begin[d] * istr[d];
    }
    lead = r > 0 && begin[0] == 0;
    expect = ext;
  } else if (b == kTflStridedSlice) {
    std::vector<int64_t> begin, end, step;
    if (!ints(1, &begin) || !ints(2, &end) || !ints(3, &step))
      return no("STRIDED_SLICE begin / end / strides must be constant int32 / int64 tensors");
    if (r > 5) return no("STRIDED_SLICE rank > 5");
    if (static_cast<int>(begin.size()) != r || static_cast<int>(end.size()) != r || static_cast<int>(step.size()) != r)
      return no("STRIDED_SLICE begin / end / strides length differs from the rank");
    const FbTable& o = op.options;
    const int begin_mask = o.valid() ? o.Int(0, 0) : 0, end_mask = o.valid() ? o.Int(1, 0) : 0;
    const int shrink_mask = o.valid() ? o.Int(4, 0) : 0;
    if (o.valid() && (o.Int(2, 0) != 0 || o.Int(3, 0) != 0))
      return no("STRIDED_SLICE ellipsis_mask / new_axis_mask unsupported");
    for (int d = 0; d < r; ++d) {
      const int64_t n = in.shape[d], s = step[d];
      if (s == 0) return no("STRIDED_SLICE stride 0");
      if (shrink_mask >> d & 1) {  // x[b]
        const int64_t i = begin[d] < 0 ? begin[d] + n : begin[d];
        if (i < 0 || i >= n) return no("STRIDED_SLICE shrink index outside the input");
        off += i * istr[d];
        continue;
      }
      // slice(b, e, s).indices(n)
      const int64_t lo = s > 0 ? 0 : -1, hi = s > 0 ? n : n - 1;
      auto bound = [&](int64_t v) {
        if (v < 0) v += n;
        return v < lo ? lo : (v > hi ? hi : v);
      };
      const int64_t start = begin_mask >> d & 1 ? (s > 0 ? 0 : n - 1) : bound(begin[d]);
      const int64_t stop = end_mask >> d & 1 ? (s > 0 ? n : -1) : bound(end[d]);
      const int64_t count = s > 0 ? (stop > start ? (stop - start + s - 1) / s : 0)
                                  : (start > stop ? (start - stop - s - 1) / -s : 0);
      if (d == 0) lead = start == 0 && s == 1;
      ext.push_back(count);
      str.push_back(s * istr[d]);
      off += (count > 0 ? start : 0) * istr[d];
    }
    expect = ext;
  } else if (b == kTflSplit || b == kTflSplitV) {
    std::vector<int64_t> axis_v, sizes;
    const bool v = b == kTflSplitV;
    if (!ints(v ? 2 : 0, &axis_v) || axis_v.size() != 1)
      return no(v ? "SPLIT_V axis must be one constant int32 / int64 value"
                  : "SPLIT axis must be one constant int32 / int64 value");
    int64_t axis = axis_v[0] < 0 ? axis_v[0] + r : axis_v[0];
    if (axis < 0 || axis >= r) return no(v ? "SPLIT_V axis out of range" : "SPLIT axis out of range");
    const int64_t n = in.shape[axis], parts = static_cast<int64_t>(op.outputs.size());
    if (op.options.valid() && op.options.Int(0, 0) != 0 && op.options.Int(0, 0) != parts)
      return no(v ? "SPLIT_V num_splits differs from the number of outputs"
                  : "SPLIT num_splits differs from the number of outputs");
    int64_t first = 0, len = 0;
    if (v) {
      if (!ints(1, &sizes)) return no("SPLIT_V size_splits must be a constant int32 / int64 tensor");
      int64_t sum = 0;
      int open = -1;
      bool bad = static_cast<int64_t>(sizes.size()) != parts;
      for (size_t k = 0; k < sizes.size() && !bad; ++k) {
        if (sizes[k] == -1 && open < 0) open = static_cast<int>(k);
        else if (sizes[k] < 0) bad = true;
        else sum += sizes[k];
      }
      if (!bad && open >= 0 && sum <= n) sizes[open] = n - sum, sum = n;
      if (bad || sum != n) return no("SPLIT_V size_splits do not sum to the axis extent");
      for (int k = 0; k < oi; ++k) first += sizes[k];
      len = sizes[oi];
    } else {
      if (n % parts != 0) return no("SPLIT axis extent is not a multiple of num_splits");
      len = n / parts;
      first = oi * len;
    }
    for (int d = 0; d < r; ++d) {
      ext.push_back(d == axis ? len : in.shape[d]);
      str.push_back(istr[d]);
    }
    off = first * istr[axis];
    lead = axis != 0;
    expect = ext;
  } else if (b == kTflUnpack) {
    if (r < 1) return no("UNPACK of a scalar");
    int64_t axis = op.options.valid() ? op.options.Int(1, 0) : 0;
    if (axis < 0) axis += r;
    if (axis < 0 || axis >= r) return no("UNPACK axis out of range");
    const int64_t parts = static_cast<int64_t>(op.outputs.size());
    if (in.shape[axis] != parts || (op.options.valid() && op.options.Int(0, 0) != 0 && op.options.Int(0, 0) != parts))
      return no("UNPACK num differs from the axis extent or the number of outputs");
    for (int d = 0; d < r; ++d) {
      if (d == axis) continue;
      ext.push_back(in.shape[d]);
      str.push_back(istr[d]);
    }
    off = oi * istr[axis];
    lead = axis != 0;
    expect = ext;
  } else if (b == kTflTile) {
    std::vector<int64_t> mult;
    if (!ints(1, &mult)) return no("TILE multiples must be a constant int32 / int64 tensor");
    if (static_cast<int>(mult.size()) != r) return no("TILE multiples length differs from the rank");
    for (int d = 0; d < r; ++d) {
      const int64_t n = in.shape[d], k = mult[d];
      if (k < 1 || k * n > std::numeric_limits<int>::max()) return no("TILE multiples must be positive");
      expect.push_back(n * k);
      // [k][n] with strides [0][s]; past axis 0 a multiple of 1 and a unit dim leave no map dim
      if (k > 1) {
        ext.push_back(k);
        str.push_back(0);
      }
      if (n > 1 || (d == 0 && k == 1)) {
        ext.push_back(n);
        str.push_back(istr[d]);
      }
    }
    if (ext.size() > BH_REINDEX_MAX_RANK)
      return no("TILE map exceeds rank 6 after unit dims and multiples of 1 are dropped");
    lead = r > 0 && mult[0] == 1;
  } else {  // SPACE_TO_DEPTH / DEPTH_TO_SPACE
    const bool d2s = b == kTflDepthToSpace;
    if (r != 4 || out.shape.size() != 4)
      return no(d2s ? "DEPTH_TO_SPACE needs 4-D tensors" : "SPACE_TO_DEPTH needs 4-D tensors");
    const int64_t bs = op.options.valid() ? op.options.Int(0, 0) : 0;
    const int64_t N = in.shape[0], H = in.shape[1], W = in.shape[2], C = in.shape[3];
    if (d2s) {
      if (bs < 1 || C % (bs * bs) != 0) return no("DEPTH_TO_SPACE block_size does not divide the channels");
      const int64_t c = C / (bs * bs);
      ext = {N, H, bs, W, bs, c};  // (n, h, by, w, bx, c)
      str = {istr[0], istr[1], bs * c, istr[2], c, 1};
      expect = {N, H * bs, W * bs, c};
    } else {
      if (bs < 1 || H % bs != 0 || W % bs != 0) return no("SPACE_TO_DEPTH block_size does not divide height and width");
      ext = {N, H / bs, W / bs, bs, bs, C};  // (n, h, w, by, bx, c)
      str = {istr[0], bs * istr[1], bs * istr[2], istr[1], istr[2], 1};
      expect = {N, H / bs, W / bs, C * bs * bs};
    }
    lead = true;
  }
  if (expect.size() != out.shape.size()) return no("output shape differs from what the op's arguments resolve to");
  const bool whole0 = lead && !out.shape.empty() && out.shape[0] == in.shape[0];
  for (size_t d = 0; d < expect.size(); ++d)
    if (out.shape[d] != expect[d] && !(d == 0 && whole0))
      return no("output shape differs from what the op's arguments resolve to");
  if (whole0) ext[0] = in.shape[0];
  if (ext.size() > BH_REINDEX_MAX_RANK) return no("rank > 6");
  *map = bh_reindex_params{};
  map->elem_bytes = static_cast<int>(GetDataTypeBytes(in.type));
  map->rank = static_cast<int>(ext.size());
  for (size_t d = 0; d < ext.size(); ++d) {
    map->out_dims[d] = static_cast<int>(ext[d]);
    map->in_stride[d] = str[d];
  }
  map->in_offset = off;
  if (whole_batch) *whole_batch = whole0;
  return true;
}

// GATHER's map for params tensor `pt` and indices tensor `it` of op (axis and
// batch_dims as given): the body of GatherArgs and of EmbeddingLookupArgs
static bool GatherBody(const TflModel& m, const TflOperator& op, int pt, int it, int axis, int batch_dims,
                       bh_gather_params* p, const char** why, bool* batch_ok) {
  auto no = [&](const char* w) {
    if (why) *why = w;
    return false;
  };
  const TflTensor& in = m.tensors[pt];
  const TflTensor& ix = m.tensors[it];
  const TflTensor& out = m.tensors[op.outputs[0]];
  if (in.type != DataType::kInt8 && in.type != DataType::kUInt8 && in.type != DataType::kFloat32 &&
      in.type != DataType::kInt32)
    return no("GATHER params must be int8, uint8, float32 or int32");
  if (out.type != in.type) return no("GATHER output type differs from params'");
  if (ix.type != DataType::kInt32 && ix.type != DataType::kInt64) return no("GATHER indices must be int32 or int64");
  if (batch_dims != 0) return no("GATHER batch_dims != 0");
  if (IsQ8(in.type) && (in.scale != out.scale || in.zero_point != out.zero_point))
    return no("GATHER output quantization differs from params' (GATHER never requantises)");
  const int r = static_cast<int>(in.shape.size());
  if (r < 1 || r > 6) return no("GATHER params rank must be 1-6");
  if (axis < 0) axis += r;
  if (axis < 0 || axis >= r) return no("GATHER axis out of range");
  std::vector<int> expect(in.shape.begin(), in.shape.begin() + axis);
  expect.insert(expect.end(), ix.shape.begin(), ix.shape.end());
  expect.insert(expect.end(), in.shape.begin() + axis + 1, in.shape.end());
  if (out.shape != expect)
    return no("GATHER output shape differs from params.shape[:axis] + indices.shape + params.shape[axis + 1:]");
  if (expect.size() > 6) return no("GATHER output rank > 6");
  bh_gather_params g{};
  g.elem_bytes = static_cast<int>(GetDataTypeBytes(in.type));
  g.index_bytes = ix.type == DataType::kInt64 ? 8 : 4;
  g.outer = g.inner = 1;
  for (int d = 0; d < axis; ++d) g.outer *= in.shape[d];
  for (int d = axis + 1; d < r; ++d) g.inner *= in.shape[d];
  g.axis_size = in.shape[axis];
  g.n_idx = static_cast<int64_t>(ix.num_elements());
  if (g.outer < 1 || g.axis_size < 1 || g.n_idx < 1 || g.inner < 1) return no("GATHER of an empty tensor");
  constexpr int64_t kMax = std::numeric_limits<int32_t>::max();
  if (g.outer > kMax || g.n_idx > kMax || g.inner > kMax || g.outer * g.n_idx > kMax ||
      g.outer * g.n_idx * g.inner > kMax / g.elem_bytes)
    return no("GATHER output of more than 2^31 - 1 bytes");
  if (ix.is_const()) {
    std::vector<int64_t> v;
    if (!ConstInts(ix, &v)) return no("GATHER constant indices are truncated");
    for (int64_t i : v)
      if (i < 0 || i >= g.axis_size) return no("GATHER constant index outside [0, axis_size)");
  }
  if (p) *p = g;
  if (batch_ok) {
    const char* w = nullptr;
    if (in.is_const()) {
      if (ix.is_const()) w = "constant params and constant indices: the output does not follow the batch axis";
      else if (axis != 0) w = "constant params gathered along an axis other than 0";
    } else {
      if (!ix.is_const()) w = "runtime indices into an activation params";
      else if (axis == 0) w = "an activation params gathered along the batch axis";
    }
    *batch_ok = w == nullptr;
    if (w && why) *why = w;
  }
  return true;
}

bool GatherArgs(const TflModel& m, const TflOperator& op, bh_gather_params* p, const char** why, bool* batch_ok) {
  if (op.builtin != kTflGather || op.inputs.size() < 2 || op.inputs[0] < 0 || op.inputs[1] < 0 || op.outputs.empty() ||
      op.outputs[0] < 0) {
    if (why) *why = "GATHER needs params, indices and an output";
    return false;
  }
  return GatherBody(m, op, op.inputs[0], op.inputs[1], op.options.valid() ? op.options.Int(0, 0) : 0,
                    op.options.valid() ? op.options.Int(1, 0) : 0, p, why, batch_ok);
}

bool EmbeddingLookupArgs(const TflModel& m, const TflOperator& op, bh_gather_params* p, const char** why,
                         bool* batch_ok) {
  auto no = [&](const char* w) {
    if (why) *why = w;
    return false;
  };
  if (op.builtin != kTflEmbeddingLookup || op.inputs.size() < 2 || op.inputs[0] < 0 || op.inputs[1] < 0 ||
      op.outputs.empty() || op.outputs[0] < 0)
    return no("EMBEDDING_LOOKUP needs ids, a table and an output");
  if (m.tensors[op.inputs[1]].type != m.tensors[op.outputs[0]].type)
    return no("EMBEDDING_LOOKUP table type differs from the output's (the dequantising form)");
  return GatherBody(m, op, op.inputs[1], op.inputs[0], 0, 0, p, why, batch_ok);
}

bool CastArgs(const TflModel& m, const TflOperator& op, int* in_type, int* out_type, const char** why) {
  auto no = [&](const char* w) {
    if (why) *why = w;
    return false;
  };
  if (op.builtin != kTflCast || op.inputs.empty() || op.inputs[0] < 0 || op.outputs.empty() || op.outputs[0] < 0)
    return no("CAST needs an input and an output");
  const TflTensor& in = m.tensors[op.inputs[0]];
  const TflTensor& out = m.tensors[op.outputs[0]];
  auto code = [](DataType t) {
    return t == DataType::kUInt8 ? BH_CAST_U8 : t == DataType::kInt32 ? BH_CAST_I32 : t == DataType::kInt64 ? BH_CAST_I64
           : t == DataType::kFloat32 ? BH_CAST_F32 : 0;
  };
  if ((IsQ8(in.type) && HasQ(in)) || (IsQ8(out.type) && HasQ(out)))
    return no("CAST of a quantized 8-bit tensor (QUANTIZE / DEQUANTIZE convert those)");
  if (!code(in.type) || !code(out.type)) return no("CAST types must be uint8, int32, int64 or float32");
  if (out.num_elements() != in.num_elements()) return no("CAST output size differs from the input's");
  if (in_type) *in_type = code(in.type);
  if (out_type) *out_type = code(out.type);
  return true;
}

bool TanhArgs(const TflModel& m, const TflOperator& op, bool* is_float, const char** why) {
  auto no = [&](const char* w) {
    if (why) *why = w;
    return false;
  };
  if (op.builtin != kTflTanh || op.inputs.empty() || op.inputs[0] < 0 || op.outputs.empty() || op.outputs[0] < 0)
    return no("TANH needs an input and an output");
  const TflTensor& in = m.tensors[op.inputs[0]];
  const TflTensor& out = m.tensors[op.outputs[0]];
  const bool f32 = in.type == DataType::kFloat32;
  if (!f32 && !IsQ8(in.type)) return no("TANH: int8, uint8 and float32 only");
  if (out.type != in.type) return no("TANH output type differs from the input's");
  if (out.num_elements() != in.num_elements()) return no("TANH output size differs from the input's");
  if (!f32 && (!HasQ(in) || !HasQ(out))) return no("TANH: missing quantization");
  if (is_float) *is_float = f32;
  return true;
}

bool PackArgs(const TflModel& m, const TflOperator& op, bh_concat_params* p, const char** why, int* axis_out) {
  auto no = [&](const char* w) {
    if (why) *why = w;
    return false;
  };
  if (op.builtin != kTflPack || op.inputs.empty() || op.outputs.empty() || op.outputs[0] < 0)
    return no("PACK needs inputs and an output");
  if (op.inputs.size() > BH_CONCAT_MAX_INPUTS) return no("PACK of more than 16 inputs");
  if (op.options.valid() && op.options.Int(0, 0) != 0 && op.options.Int(0, 0) != static_cast<int>(op.inputs.size()))
    return no("PACK values_count differs from the number of inputs");
  for (int t : op.inputs)
    if (t < 0) return no("PACK needs inputs and an output");
  const TflTensor& x0 = m.tensors[op.inputs[0]];
  const TflTensor& out = m.tensors[op.outputs[0]];
  if (out.type != DataType::kInt8 && out.type != DataType::kUInt8 && out.type != DataType::kFloat32 &&
      out.type != DataType::kInt32)
    return no("PACK element type must be int8, uint8, float32 or int32");
  const int r = static_cast<int>(x0.shape.size());
  int axis = op.options.valid() ? op.options.Int(1, 0) : 0;
  if (axis < 0) axis += r + 1;
  if (axis < 0 || axis > r) return no("PACK axis out of range");
  for (int t : op.inputs) {
    const TflTensor& x = m.tensors[t];
    if (x.type != out.type || x.shape != x0.shape) return no("PACK inputs must share one shape and the output's type");
    if (IsQ8(out.type) && (x.scale != out.scale || x.zero_point != out.zero_point))
      return no("PACK inputs must share the output's quantization (pack.cc)");
  }
  std::vector<int> expect = x0.shape;
  expect.insert(expect.begin() + axis, static_cast<int>(op.inputs.size()));
  if (out.shape != expect) return no("PACK output shape is not the stacked shape");
  long outer = 1, row = static_cast<long>(GetDataTypeBytes(out.type));
  for (int d = 0; d < axis; ++d) outer *= x0.shape[d];
  for (int d = axis; d < r; ++d) row *= x0.shape[d];
  if (outer < 1 || row < 1) return no("PACK of empty tensors");
  if (outer * row * static_cast<long>(op.inputs.size()) >= std::numeric_limits<int32_t>::max())
    return no("PACK output of 2^31 - 1 or more bytes");
  if (p) {
    *p = bh_concat_params{};
    p->n_inputs = static_cast<int>(op.inputs.size());
    p->outer = outer;
    for (int k = 0; k < p->n_inputs; ++k) p->row[k] = row;
  }
  if (axis_out) *axis_out = axis;
  return true;
}

bool DetectionSupported(const TflModel& m, const TflOperator& op, CpuDetectionParams* p,
                        int* batch) {
  if (op.builtin != kTflCustom || op.custom_code != "TFLite_Detection_PostProcess") return false;
  if (op.inputs.size() != 3 || op.outputs.size() != 4) return false;
  for (int t : op.inputs)
    if (t < 0) return false;
  const TflTensor& be = m.tensors[op.inputs[0]];
  const TflTensor& cs = m.tensors[op.inputs[1]];
  const TflTensor& an = m.tensors[op.inputs[2]];
  if (be.type != DataType::kFloat32 || cs.type != DataType::kFloat32 || an.type != DataType::kFloat32 ||
      !an.is_const())
    return false;
  FlexMap f;
  if (!f.Parse(op.custom_options, op.custom_options_size)) return false;
  if (f.Number("use_regular_nms", 0) != 0 || f.Number("max_classes_per_detection", 1) != 1) return false;
  const int n = an.shape.empty() ? 0 : an.shape[0];
  if (n <= 0 || be.num_elements() == 0 || be.num_elements() % (static_cast<size_t>(n) * 4)) return false;
  const size_t images = be.num_elements() / (static_cast<size_t>(n) * 4);
  if ((images != 1 && !batch) || images > (1u << 16) || cs.num_elements() % (images * n)) return false;
  CpuDetectionParams d{};
  d.num_boxes = n;
  d.num_classes = static_cast<int>(f.Number("num_classes", 0));
  d.num_classes_with_background = static_cast<int>(cs.num_elements() / (images * n));
  d.max_detections = static_cast<int>(f.Number("max_detections", 0));
  // options are read with AsFloat (float), detection_postprocess.cc Init()
  d.score_threshold = static_cast<float>(f.Number("nms_score_threshold", 0));
  d.iou_threshold = static_cast<float>(f.Number("nms_iou_threshold", 0));
  d.scale_y = static_cast<float>(f.Number("y_scale", 0));
  d.scale_x = static_cast<float>(f.Number("x_scale", 0));
  d.scale_h = static_cast<float>(f.Number("h_scale", 0));
  d.scale_w = static_cast<float>(f.Number("w_scale", 0));
  if (d.num_classes <= 0 || d.num_classes > d.num_classes_with_background || d.max_detections <= 0) return false;
  for (int k = 0; k < 4; ++k)
    if (m.tensors[op.outputs[k]].type != DataType::kFloat32) return false;
  const size_t rows = images * static_cast<size_t>(d.max_detections);
  if (m.tensors[op.outputs[0]].num_elements() != rows * 4 || m.tensors[op.outputs[1]].num_elements() != rows ||
      m.tensors[op.outputs[2]].num_elements() != rows || m.tensors[op.outputs[3]].num_elements() != images)
    return false;
  if (p) *p = d;
  if (batch) *batch = static_cast<int>(images);
  return true;
}

}  // namespace ex
}  // namespace hip
}  // namespace band
