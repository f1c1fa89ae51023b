// One Args function per op family: it resolves an op's shapes and options,
// applies the limits of the kernels and names what it refuses.  The support
// checks (GpuSupports / FloatSupports), the lowering (lower.cc) and the
// job-batch rule (model.cc) all call the same function, so what a worker
// accepts is what the lowering can handle.  Needs only the TFLite reader and
// quant.cc: no device, no executor.
#pragma once

#include <cstdint>
#include <vector>

#include "backend/hip/cpu_kernels.h"
#include "backend/hip/quant.h"
#include "backend/hip/tflite_reader.h"
#include "band_hip_kernels.h"

namespace band {
namespace hip {
namespace ex {

inline bool IsQ8(DataType t) { return t == DataType::kInt8 || t == DataType::kUInt8; }

// zero point in the kernels' int8 domain (uint8 values are XOR 0x80 = x-128)
inline int32_t Dom(const TflTensor& t) {
  const int32_t zp = t.zero_point.empty() ? 0 : static_cast<int32_t>(t.zero_point[0]);
  return t.type == DataType::kUInt8 ? zp - 128 : zp;
}
inline int32_t Zp(const TflTensor& t) { return t.zero_point.empty() ? 0 : static_cast<int32_t>(t.zero_point[0]); }
inline float Scale(const TflTensor& t) { return t.scale.empty() ? 0.0f : t.scale[0]; }
inline bool HasQ(const TflTensor& t) { return !t.scale.empty(); }

inline void Shape4(const std::vector<int>& s, int* out) {
  const int pad = 4 - static_cast<int>(s.size());
  for (int i = 0; i < 4; ++i) out[i] = i < pad ? 1 : s[i - pad];
}

// TFLite fp16 post-training quantization keeps constants in float16 behind
// DEQUANTIZE ops; such a tensor is a constant of the float graph
const TflOperator* ProducerOf(const TflModel& m, int t);
bool FoldableF16(const TflModel& m, int t);
inline bool ConstFloat(const TflModel& m, int t) {
  return t >= 0 && ((m.tensors[t].is_const() && m.tensors[t].type == DataType::kFloat32) || FoldableF16(m, t));
}

// CONV_2D (dense and grouped), DEPTHWISE_CONV_2D and TRANSPOSE_CONV, int8 /
// uint8 and float32.  TRANSPOSE_CONV: in_* is the op's input, out_* its output
// tensor (not the constant output_shape input: a job-batch variant scales axis
// 0 of tensors, not of constants); pad_* as transpose_conv.cc computes it, for
// a conv whose input is the output.
struct ConvGeometry {
  int batch, in_h, in_w, in_c, out_h, out_w, out_c;
  int k_h, k_w, stride_h, stride_w, dil_h, dil_w, pad_h, pad_w;
  int act;               // schema ActivationFunctionType
  int groups;            // CONV_2D: in_c / the filter's input channels
  int depth_multiplier;  // DEPTHWISE_CONV_2D: out_c / in_c
  int filter, input, bias;  // tensor indices; bias -1: none
};
// g may be null (a pure check); *why names what was refused
bool ConvArgs(const TflModel& m, const TflOperator& op, ConvGeometry* g, const char** why = nullptr);

// FULLY_CONNECTED: input viewed as [rows][depth], filter [units][depth]
struct FcGeometry {
  int rows, depth, units, act;
  int filter, bias;  // tensor indices; bias -1: none
};
bool FcArgs(const TflModel& m, const TflOperator& op, FcGeometry* g, const char** why = nullptr);

// A float32 op whose filter is 8-bit: the converter's dynamic-range ("hybrid")
// form.  FULLY_CONNECTED runs (HybridFcArgs); CONV_2D and DEPTHWISE_CONV_2D
// run on executors built with BAND_HIP_HYBRID_CONV=1 (HybridConvArgs) and are
// refused by name on every other.
inline bool IsHybridWeightOp(const TflModel& m, const TflOperator& op) {
  return (op.builtin == kTflFullyConnected || op.builtin == kTflConv2D || op.builtin == kTflDepthwiseConv2D) &&
         op.inputs.size() >= 2 && op.inputs[0] >= 0 && op.inputs[1] >= 0 &&
         m.tensors[op.inputs[0]].type == DataType::kFloat32 && IsQ8(m.tensors[op.inputs[1]].type);
}
// Hybrid FULLY_CONNECTED: FcArgs' geometry, the filter's one scale and
// FullyConnectedOptions.asymmetric_quantize_inputs (slot 3).  Refused with a
// reason that names the op: per-channel filter scales, a non-zero filter zero
// point, a uint8 or non-constant filter, weights_format != 0, a bias that is
// not a float constant, a non-float32 output, depth > 65,535 (the int32 dot).
// Every row is quantised alone, so a job-batch variant (more rows) computes
// each job's own values.
struct HybridFcGeometry {
  FcGeometry fc;
  float w_scale;
  bool asymmetric;
};
bool HybridFcArgs(const TflModel& m, const TflOperator& op, HybridFcGeometry* g, const char** why = nullptr);

inline bool IsHybridConvOp(const TflModel& m, const TflOperator& op) {
  return op.builtin != kTflFullyConnected && IsHybridWeightOp(m, op);
}
// Hybrid CONV_2D / DEPTHWISE_CONV_2D: ConvArgs' geometry, the filter scales
// expanded to [out_c] and the form.  The scale count selects the form, nothing
// in the flatbuffer does: one scale (CONV_2D only) quantises the input
// symmetrically and ends in bias + acc * (s * ws); out_c scales (quantised
// dimension 0, 3 for depthwise) quantise it asymmetrically and end in
// (acc * ws[c]) * s + bias (conv) or acc * (ws[c] * s) + bias (depthwise).
// Refused with a reason that names the op: a uint8 or non-constant filter, a
// bias that is not a float32 constant, a non-float32 output, a non-zero
// filter zero point, a scale count that is neither 1 nor out_c, one scale on a
// depthwise filter, a non-positive scale, a grouped filter, k_h k_w in_c >
// 65,535 (the int32 sum), a tensor of 2^31 or more elements, and whatever
// ConvArgs refuses.  Every batch item is quantised alone, so a job-batch
// variant (more items) computes each job's own values.
struct HybridConvGeometry {
  ConvGeometry conv;
  bool depthwise;
  bool per_channel;  // out_c scales: the asymmetric input quantisation
  std::vector<float> w_scale;  // [out_c]
};
bool HybridConvArgs(const TflModel& m, const TflOperator& op, HybridConvGeometry* g, const char** why = nullptr);

// AVERAGE_POOL_2D / MAX_POOL_2D
struct PoolGeometry {
  int batch, in_h, in_w, channels, out_h, out_w;
  int f_h, f_w, stride_h, stride_w, pad_h, pad_w, act;
};
bool PoolArgs(const TflModel& m, const TflOperator& op, PoolGeometry* g, const char** why = nullptr);

// the rank-4 shapes of a binary op's operands and output; each operand dim is
// the output's or 1
struct BroadcastShapes {
  int a[4], b[4], o[4];
};
bool BroadcastArgs(const TflModel& m, const TflOperator& op, BroadcastShapes* s, const char** why = nullptr);

// BATCH_MATMUL (int8 / float32): shapes, adj_x / adj_y and numpy-matmul
// broadcasting of the leading dims resolved to the stride form of
// bh_batch_matmul_params (pointers stay null) - the only place that does; the
// support checks, the lowering, the host twin's caller and the job-batch rule
// all come through here.  int8: one per-tensor (mult, shift) from
// FullyConnectedMultiplier, the zero points of both operands and the output.
// *batch_axis_ok: axis 0 of the output and of every non-constant operand is
// the same matmul batch dim (rank >= 3, the output's rank) and a constant
// operand broadcasts along it (lower rank, or a leading 1), so a job-batch
// variant that scales axis 0 computes each job's product.  *why names what
// was refused.
bool BatchMatMulArgs(const TflModel& m, const TflOperator& op, bh_batch_matmul_params* p,
                     const char** why = nullptr, bool* batch_axis_ok = nullptr);

// MIRROR_PAD paddings (constant [rank][2] int32 / int64) and mode
// (MirrorPadOptions.mode: 0 REFLECT, 1 SYMMETRIC -> bh_pad_params.mode 1 / 2)
bool MirrorPadArgs(const TflModel& m, const TflOperator& op, std::vector<int64_t>* pads, int* mode);

// MEAN: the reduced axes (constant int32, negatives resolved) must be one
// contiguous run; 8-bit tensors only in the form TFLite 2.9.2 runs through
// optimized_integer_ops::Mean / optimized_ops::Mean (4-D, keep_dims, axes
// {1, 2}), the one restated by CpuMean - or, `rows`, over the last axis alone
// (rank 1-4, keep_dims either way), the other two branches of reduce.cc
// EvalMean, restated by CpuMeanRows / mean_rows_kernel: `exact` when input and
// output share scale and zero point (reference_ops::Mean), else
// reference_ops::QuantizedMeanOrSum.  *why names what was refused.
struct MeanGeometry {
  long outer, reduce, inner;  // the input viewed as [outer][reduce][inner]
  bool rows;                  // 8-bit, last axis: [outer][reduce], inner 1
  bool exact;                 // 8-bit: input and output quantisation are equal
  bool reduces_axis0;         // the job-batch rule: axis 0 is among the reduced ones
};
bool MeanArgs(const TflModel& m, const TflOperator& op, MeanGeometry* g, const char** why = nullptr);
bool MeanArgs(const TflModel& m, const TflOperator& op, long* outer, long* reduce, long* inner);

// SQUARED_DIFFERENCE int8: BroadcastArgs' shapes and squared_difference.cc's
// multipliers (SquaredDifferenceParams); uint8 / int16 and an output
// multiplier >= 1 are refused with a reason
bool SquaredDifferenceArgs(const TflModel& m, const TflOperator& op, BroadcastShapes* s, AddParams* q,
                           const char** why = nullptr);

// ARG_MAX / ARG_MIN (arg_min_max.cc): int8 / uint8 / float32 input of rank
// 1-4 viewed as [outer][axis_len][inner]; the axis is a constant int32 /
// int64 scalar or one-element tensor (negatives resolved); the output is
// int32 or int64 as ArgMaxOptions / ArgMinOptions.output_type says, with
// outer * inner elements.  *why (optional) names what failed.
bool ArgMinMaxArgs(const TflModel& m, const TflOperator& op, long* outer, long* axis_len, long* inner,
                   int* out_bytes, int* axis_out = nullptr, const char** why = nullptr);

// The re-indexing ops: TRANSPOSE, STRIDED_SLICE, SLICE, SPLIT, SPLIT_V,
// SPACE_TO_DEPTH, DEPTH_TO_SPACE, UNPACK, TILE
inline bool IsReindexOp(int builtin) {
  return builtin == kTflTranspose || builtin == kTflStridedSlice || builtin == kTflSlice || builtin == kTflSplit ||
         builtin == kTflSplitV || builtin == kTflSpaceToDepth || builtin == kTflDepthToSpace ||
         builtin == kTflUnpack || builtin == kTflTile;
}
// the values of a constant int32 / int64 tensor
bool ConstInts(const TflTensor& t, std::vector<int64_t>* v);

// Resolves output `oi` of a re-indexing op to the map bh_reindex / CpuReindex
// run (map->input / output stay null): the output's extents (rank <= 6),
// signed input strides in elements and an input element offset.  Semantics
// are numpy's: np.transpose(x, perm); x[b:b+s] per axis with size -1 = to the
// end; basic indexing x[b:e:s] per axis (negative indices, out-of-range
// clamping, negative strides; a begin_mask / end_mask bit makes the bound None,
// a shrink_axis_mask bit makes the axis the index x[b]); np.split;
// DEPTH_TO_SPACE out[n, h bs + by, w bs + bx, c] = in[n, h, w, (by bs + bx) C' + c]
// and SPACE_TO_DEPTH its inverse; UNPACK output k is np.moveaxis(x, axis, 0)[k]
// (the SPLIT map with the axis dropped); np.tile(x, multiples) with constant
// multiples - input dim d with multiple m > 1 becomes the two map dims [m][d]
// with input strides [0][s], unit dims and multiples of 1 past axis 0 leave no
// map dim, and what is left must fit rank 6.  Starts and strides come from the constants
// and the input's shape, extents from the OUTPUT tensor's shape, which must be
// what the constants resolve to - except that an output may take the whole of
// input axis 0 from element 0 at stride 1 whatever end / size say (a job-batch
// variant scales axis 0 of every tensor, not the constants).  *whole_batch:
// the output's axis 0 is the input's, in full (the job-batch rule).  *why names
// what was refused.
bool ReindexArgs(const TflModel& m, const TflOperator& op, int oi, bh_reindex_params* map,
                 const char** why = nullptr, bool* whole_batch = nullptr);

// GATHER (gather.cc, batch_dims 0): params viewed as [outer][axis_size][inner]
// (GatherOptions.axis, negatives resolved), the indices flattened to n_idx -
// p's counts, elem_bytes and index_bytes (pointers stay null); p may be null
// (a pure check).  params is int8 / uint8 / float32 / int32 of rank 1-6, a
// constant or an activation; indices int32 / int64, a constant or a runtime
// tensor.  Refused with a reason: batch_dims != 0, 8-bit params whose output
// quantisation differs (GATHER never requantises), an output shape other than
// params.shape[:axis] + indices.shape + params.shape[axis + 1:] or of rank > 6,
// more than 2^31 - 1 output bytes, a constant index outside [0, axis_size).
// *batch_ok: a job-batch variant (axis 0 of every non-constant tensor scaled)
// computes each job's own rows - constant params gathered along axis 0 by
// runtime indices (the embedding), or an activation params gathered along an
// axis >= 1 by constant indices; when the op is accepted and *batch_ok is
// false, *why names what keeps it from batching.
bool GatherArgs(const TflModel& m, const TflOperator& op, bh_gather_params* p, const char** why = nullptr,
                bool* batch_ok = nullptr);
// EMBEDDING_LOOKUP (embedding_lookup.cc): inputs (ids, table); GATHER's map
// with axis 0 and the operands exchanged, through the same body - the same
// refusals (their reasons say GATHER), the same out-of-range rule, the same
// job-batch rule.  A table whose type differs from the output's (TFLite's
// dequantising form) is refused.
bool EmbeddingLookupArgs(const TflModel& m, const TflOperator& op, bh_gather_params* p, const char** why = nullptr,
                         bool* batch_ok = nullptr);
// (params, indices) operand positions of a GATHER / an EMBEDDING_LOOKUP
inline void GatherOperands(const TflOperator& op, int* params, int* indices) {
  *params = op.builtin == kTflEmbeddingLookup ? 1 : 0;
  *indices = 1 - *params;
}
// CAST (cast.cc): the BH_CAST_* codes of the input and output tensors' types (uint8, int32, int64, float32; the
// options are not read), equal element counts.  A quantised 8-bit tensor (one that has scales) is refused:
// its values are QUANTIZE's / DEQUANTIZE's to convert.  Elementwise: job batching needs no rule of its own.
bool CastArgs(const TflModel& m, const TflOperator& op, int* in_type = nullptr, int* out_type = nullptr,
              const char** why = nullptr);
// TANH (activations.cc): int8 / uint8 with quantisation (a 256-entry table,
// TanhTable) or float32 (BH_UNARY_TANH); elementwise, equal sizes and types
bool TanhArgs(const TflModel& m, const TflOperator& op, bool* is_float = nullptr, const char** why = nullptr);

// PACK (pack.cc; np.stack): the bh_concat launch of its inputs - outer the
// product of the dims before the axis, row[k] the bytes of one input's
// remainder (pointers stay null); p may be null.  Refused with a reason: more
// than BH_CONCAT_MAX_INPUTS inputs, inputs that differ in shape or type,
// 8-bit inputs without the output's quantisation, an output that is not the
// stacked shape.  *axis: the resolved axis (0: the batch axis).
bool PackArgs(const TflModel& m, const TflOperator& op, bh_concat_params* p, const char** why = nullptr,
              int* axis = nullptr);

// TFLite_Detection_PostProcess in the form the host kernel and the device
// kernels (kernels/detection.hip) implement.  batch: the images of a
// job-batch variant (the leading dimension of the op's tensors; the anchors
// are shared) - without it only one image is accepted.
bool DetectionSupported(const TflModel& m, const TflOperator& op, CpuDetectionParams* p, int* batch = nullptr);

}  // namespace ex
}  // namespace hip
}  // namespace band
