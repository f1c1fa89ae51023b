// Launch: one record of a prepared subgraph's launch program - a kind, the one
// parameter block (payload) that kind carries, and what the profiler reports.
// Includes nothing of the executor.  The kind -> call table of both workers is
// in model_executor.cc (kCalls).
//
// A new kind is an enum entry, a row of kPayloads (and a Payload alternative
// when no existing block fits) and a row of kCalls; the static_asserts below
// and next to kCalls refuse a build that misses one.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <type_traits>
#include <utility>
#include <variant>
#include <vector>

#include "backend/hip/cpu_kernels.h"
#include "band_hip_kernels.h"

namespace band {
namespace hip {

// the payloads of the kinds whose launcher takes loose arguments
// kCopy; nothing moves when src == dst.  cast_to != 0: a converting copy (CAST): `count` elements of BH_CAST_* type
// cast_from at src are written as cast_to at dst (bh_cast / CpuCast), and `bytes` is the output's size.  CAST has no
// kind of its own: it is a copy that changes the element type.
struct CopyArgs {
  void* dst;
  const void* src;
  size_t bytes;
  int cast_from = 0, cast_to = 0;
  long count = 0;
};
struct LutArgs {  // kLutU8 / kLutF32: `count` bytes through a 256-entry device table of bytes / floats
  const void* src;
  void* dst;
  long count;
  const void* table;
};
struct QuantF32Args {  // kQuantF32: `count` floats to int8 (is_signed) / uint8
  const float* src;
  void* dst;
  long count;
  float scale;
  int32_t zp;
  int is_signed;
};
struct UnaryF32Args {  // kUnaryF32: BH_UNARY_* `kind` over `count` floats; lo / hi for BH_UNARY_CLAMP
  int kind;
  const float* src;
  float* dst;
  long count;
  float lo, hi;
};
struct SoftmaxF32Args {  // kSoftmaxF32 over the last axis: rows x depth
  const float* src;
  float* dst;
  long rows;
  int depth;
  float beta;
};
struct ConvGroupArgs {  // kConvGroup: the member convs (program order) and the planned group
  std::vector<bh_conv_params> members;
  bh_conv_group cgroup;
};

// kLayerNorm: bh_layernorm_params carries the ten blocks of the ops it replaces
// (1,056 bytes, the one block larger than bh_chain_params), so it lives outside
// the record.  FuseLayerNorm makes it whole and nothing changes it afterwards;
// copies of the launch share it.
struct LayerNormArgs {
  std::shared_ptr<const bh_layernorm_params> p;
};

namespace launch_detail {
template <class T, class V>
struct IndexIn;
template <class T, class... Ts>
struct IndexIn<T, std::variant<Ts...>> {
  static constexpr size_t Find() {
    const bool same[] = {std::is_same<T, Ts>::value...};
    for (size_t i = 0; i < sizeof...(Ts); ++i)
      if (same[i]) return i;
    return sizeof...(Ts);
  }
  static constexpr size_t value = Find();
  static_assert(value < sizeof...(Ts), "not a launch payload");
};
}  // namespace launch_detail

class Launch {
 public:
  enum Kind {
    kConv, kDwConv, kFc, kEltwise, kPool, kCopy, kIrb, kChain,
    kLutU8, kLutF32, kQuantF32, kConcat, kPad, kResizeNearest, kResizeBilinear, kSoftmax, kZeroInsert,
    kConvF32, kFcF32, kEltwiseF32, kPoolF32, kUnaryF32, kSoftmaxF32,  // float32 graphs
    kResizeBilinearU8,
    kDetectionPost,  // CPU-only TFLite_Detection_PostProcess
    kMean,           // MEAN: float32 over a run of axes, 8-bit over H, W
    kMeanRows,       // MEAN of an 8-bit tensor over its last axis
    kConvGroup,      // independent small convs in one dispatch (GroupConvs)
    kDetectionGpu,   // TFLite_Detection_PostProcess on the device (BAND_HIP_GPU_DETECTION=1)
    kArgMinMax,      // ARG_MAX / ARG_MIN
    kResizeArgMinMax, // RESIZE_BILINEAR int8 -> ARG_MAX / ARG_MIN over channels, one launch (FuseGlue; kGPU)
    kReindex,         // one output of TRANSPOSE / STRIDED_SLICE / SLICE / SPLIT / SPLIT_V / SPACE_TO_DEPTH / DEPTH_TO_SPACE / UNPACK / TILE, or a GATHER (a map with indices)
    kConvGrouped,     // grouped CONV_2D: the dense block with the total channel counts + groups (never chained / grouped / blocked)
    kBatchMatMul,     // BATCH_MATMUL int8 (BatchMatMulArgs; never chained / grouped / blocked, no epilogue folds)
    kBatchMatMulF32,  // BATCH_MATMUL float32
    kLayerNorm,       // the ten ops of an int8 LayerNorm as one launch (FuseLayerNorm; kGPU)
    kAttention,       // BATCH_MATMUL -> [ADD of a mask / bias] -> SOFTMAX -> BATCH_MATMUL (int8) as one launch (FuseAttention; kGPU, opt-in)
    kDynQuantRows,    // hybrid FULLY_CONNECTED, first launch: the input's rows quantised into the subgraph's scratch
    kFcHybrid,        // hybrid FULLY_CONNECTED, second launch: int8 product, float epilogue
    kDynQuantItems,   // hybrid CONV_2D / DEPTHWISE_CONV_2D, first launch(es): each batch item quantised into the subgraph's scratch
    kConvHybrid,      // hybrid CONV_2D: int8 implicit GEMM, float epilogue
    kDwConvHybrid,    // hybrid DEPTHWISE_CONV_2D
    kLayerNormF32,    // the ten ops of a float32 LayerNorm as one launch, with the row quantisation of the hybrid
                      // FULLY_CONNECTEDs that read it (FuseLayerNormF32 / FoldLayerNormQuant; kGPU, opt-in)
    kNumKinds,
    kNone = kNumKinds  // no payload yet: not runnable, never emitted
  };
  using Payload =
      std::variant<std::monostate, bh_conv_params, bh_conv_grouped_params, bh_dwconv_params, bh_fc_params,
                   bh_eltwise_params, bh_pool_params, CopyArgs, bh_irb_params, bh_chain_params, LutArgs, QuantF32Args,
                   bh_concat_params, bh_pad_params, bh_resize_nearest_params, bh_resize_bilinear_params,
                   bh_softmax_params, bh_zero_insert_params, bh_conv_f32_params, bh_fc_f32_params,
                   bh_eltwise_f32_params, bh_pool_f32_params, UnaryF32Args, SoftmaxF32Args,
                   bh_resize_bilinear_u8_params, CpuDetectionParams, bh_mean_params, bh_mean_rows_params, ConvGroupArgs,
                   bh_detection_params, bh_argminmax_params, bh_resize_argminmax_params, bh_reindex_params,
                   bh_batch_matmul_params, LayerNormArgs, bh_attention_params, bh_dynquant_params,
                   bh_fc_hybrid_params, bh_dynquant_items_params, bh_conv_hybrid_params, bh_layernorm_f32_params>;
  template <class P>
  static constexpr size_t kIndex = launch_detail::IndexIn<P, Payload>::value;

  // the one payload type of every kind, in enum order
  struct PayloadRow {
    Kind kind;
    size_t index;  // of Payload
  };
  static constexpr PayloadRow kPayloads[] = {
      {kConv, kIndex<bh_conv_params>},
      {kDwConv, kIndex<bh_dwconv_params>},
      {kFc, kIndex<bh_fc_params>},
      {kEltwise, kIndex<bh_eltwise_params>},
      {kPool, kIndex<bh_pool_params>},
      {kCopy, kIndex<CopyArgs>},
      {kIrb, kIndex<bh_irb_params>},
      {kChain, kIndex<bh_chain_params>},
      {kLutU8, kIndex<LutArgs>},
      {kLutF32, kIndex<LutArgs>},
      {kQuantF32, kIndex<QuantF32Args>},
      {kConcat, kIndex<bh_concat_params>},
      {kPad, kIndex<bh_pad_params>},
      {kResizeNearest, kIndex<bh_resize_nearest_params>},
      {kResizeBilinear, kIndex<bh_resize_bilinear_params>},
      {kSoftmax, kIndex<bh_softmax_params>},
      {kZeroInsert, kIndex<bh_zero_insert_params>},
      {kConvF32, kIndex<bh_conv_f32_params>},
      {kFcF32, kIndex<bh_fc_f32_params>},
      {kEltwiseF32, kIndex<bh_eltwise_f32_params>},
      {kPoolF32, kIndex<bh_pool_f32_params>},
      {kUnaryF32, kIndex<UnaryF32Args>},
      {kSoftmaxF32, kIndex<SoftmaxF32Args>},
      {kResizeBilinearU8, kIndex<bh_resize_bilinear_u8_params>},
      {kDetectionPost, kIndex<CpuDetectionParams>},
      {kMean, kIndex<bh_mean_params>},
      {kMeanRows, kIndex<bh_mean_rows_params>},
      {kConvGroup, kIndex<ConvGroupArgs>},
      {kDetectionGpu, kIndex<bh_detection_params>},
      {kArgMinMax, kIndex<bh_argminmax_params>},
      {kResizeArgMinMax, kIndex<bh_resize_argminmax_params>},
      {kReindex, kIndex<bh_reindex_params>},
      {kConvGrouped, kIndex<bh_conv_grouped_params>},
      {kBatchMatMul, kIndex<bh_batch_matmul_params>},
      {kBatchMatMulF32, kIndex<bh_batch_matmul_params>},
      {kLayerNorm, kIndex<LayerNormArgs>},
      {kAttention, kIndex<bh_attention_params>},
      {kDynQuantRows, kIndex<bh_dynquant_params>},
      {kFcHybrid, kIndex<bh_fc_hybrid_params>},
      {kDynQuantItems, kIndex<bh_dynquant_items_params>},
      {kConvHybrid, kIndex<bh_conv_hybrid_params>},
      {kDwConvHybrid, kIndex<bh_conv_hybrid_params>},
      {kLayerNormF32, kIndex<bh_layernorm_f32_params>},
  };
  template <Kind K>
  using PayloadOf = std::variant_alternative_t<kPayloads[K].index, Payload>;

  int op_index = -1;
  int out_tensor = -1;   // tensor this launch materialises (after epilogue fusions)
  double alg_bytes = 0;  // algorithmic HBM bytes per launch (roofline numerator)
  double alg_ops = 0;    // algorithmic int ops (2 per MAC)
  const char* kernel = "";

  Kind kind() const { return kind_; }

  // The one way a launch gets its kind and its payload (replacing what it
  // held): Set<K>(p) takes kind K's payload type alone; Set(k, p), for a kind
  // chosen at run time, stops the process unless p is kind k's payload type.
  // Both return the stored payload, for the caller to fill.
  template <Kind K>
  PayloadOf<K>& Set(PayloadOf<K> p = {}) {
    kind_ = K;
    return payload_.template emplace<PayloadOf<K>>(std::move(p));
  }
  template <class P>
  P& Set(Kind k, P p) {
    if (k < 0 || k >= kNumKinds || kPayloads[k].index != kIndex<P>) Mismatch(k, kIndex<P>);
    kind_ = k;
    return payload_.template emplace<P>(std::move(p));
  }

  // the payload as a P: null when the launch holds another type ...
  template <class P>
  P* get_if() { return std::get_if<P>(&payload_); }
  template <class P>
  const P* get_if() const { return std::get_if<P>(&payload_); }
  // ... or the process stops, naming the launch
  template <class P>
  P& as() {
    if (P* p = get_if<P>()) return *p;
    Mismatch(kind_, kIndex<P>);
  }
  template <class P>
  const P& as() const { return const_cast<Launch*>(this)->as<P>(); }

  // the dense conv block of a kConv or a kConvGrouped launch: LaunchIo, the
  // epilogue folds and the residual ADD treat the two alike
  bh_conv_params* conv_if() {
    if (bh_conv_grouped_params* g = get_if<bh_conv_grouped_params>()) return &g->conv;
    return get_if<bh_conv_params>();
  }
  const bh_conv_params* conv_if() const { return const_cast<Launch*>(this)->conv_if(); }
  bh_conv_params& conv() {
    if (bh_conv_params* c = conv_if()) return *c;
    Mismatch(kind_, kIndex<bh_conv_params>);
  }
  const bh_conv_params& conv() const { return const_cast<Launch*>(this)->conv(); }

 private:
  [[noreturn]] void Mismatch(int kind, size_t wanted) const {
    std::fprintf(stderr, "Launch %s: kind %d (payload %zu) taken as kind %d with payload %zu\n", kernel,
                 static_cast<int>(kind_), payload_.index(), kind, wanted);
    std::abort();
  }

  Kind kind_ = kNone;
  Payload payload_;
};

namespace launch_detail {
constexpr bool PayloadRowsInOrder() {
  for (int k = 0; k < Launch::kNumKinds; ++k)
    if (Launch::kPayloads[k].kind != k || Launch::kPayloads[k].index == 0) return false;
  return true;
}
}  // namespace launch_detail
static_assert(sizeof(Launch::kPayloads) / sizeof(Launch::kPayloads[0]) == Launch::kNumKinds, "one payload row per kind");
static_assert(launch_detail::PayloadRowsInOrder(), "kPayloads row i names kind i and a payload");
// the largest payload, the variant's index and the 40 bytes of the other fields
static_assert(sizeof(Launch) <= sizeof(bh_chain_params) + 64, "a payload outgrew bh_chain_params: hold it outside the record, as LayerNormArgs does");

}  // namespace hip
}  // namespace band
