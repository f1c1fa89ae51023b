// HipModelExecutor: lowering of TFLite ops to kernel launches (Launch records)
// - the per-op parameter derivation, constants packed and uploaded once per
// (model, GPU), the residual-ADD epilogue fold.  Split from model_executor.cc.
#include "backend/hip/executor_internal.h"

namespace band {
namespace hip {

using namespace ex;

namespace {

// what an int8 / uint8 conv's epilogue needs: per-channel multipliers, the
// clamp, the zero points in the kernels' int8 domain and the bias
struct ConvQuant {
  std::vector<int32_t> mult, shift;
  int32_t amin, amax, in_zp, w_zp;
  const int32_t* bias;
};

ConvQuant QuantOf(const TflModel& d, const ConvGeometry& g, const TflTensor& out) {
  const TflTensor& in = d.tensors[g.input];
  const TflTensor& w = d.tensors[g.filter];
  const bool i8 = in.type == DataType::kInt8;
  ConvQuant q;
  ConvMultipliers(Scale(in), w.scale, g.out_c, Scale(out), !i8, &q.mult, &q.shift);
  ActivationRangeQuantized(g.act, Scale(out), Zp(out), i8, &q.amin, &q.amax);
  q.in_zp = Dom(in);
  q.w_zp = i8 ? 0 : Dom(w);  // int8 kernels ignore the filter zero point
  q.bias = g.bias >= 0 ? reinterpret_cast<const int32_t*>(d.tensors[g.bias].data) : nullptr;
  return q;
}

// A 1x1 stride-1 conv over a handful of pixels (the classifier at batch 1)
// is a GEMV: it runs on the weight-streaming FC kernel with the same packed
// operands (Bt rows are K-contiguous, bias_eff identical).  True when *L was
// rewritten.
bool GemvAsFc(Launch* L) {
  const bh_conv_params c = L->as<bh_conv_params>();
  const long M = static_cast<long>(c.batch) * c.out_h * c.out_w;
  if (c.k_h != 1 || c.k_w != 1 || c.stride_h != 1 || c.stride_w != 1 || M > 4) return false;
  Launch F;
  F.op_index = L->op_index;
  F.out_tensor = L->out_tensor;
  bh_fc_params& f = F.Set<Launch::kFc>();
  f.rows = static_cast<int>(M); f.depth = c.in_c; f.depth_pad = c.k_pad; f.units = c.out_c;
  f.in_xor = c.in_xor; f.in_zp = c.in_zp; f.w_zp = c.w_zp; f.out_zp = c.out_zp;
  f.act_min = c.act_min; f.act_max = c.act_max; f.input = c.input; f.output = c.output;
  f.weights = c.weights; f.bias_eff = c.bias_eff; f.mult = c.mult; f.shift = c.shift;
  F.kernel = "fc_kernel";
  F.alg_bytes = L->alg_bytes;
  F.alg_ops = L->alg_ops;
  *L = F;
  return true;
}

// the geometry fields bh_conv_params, bh_dwconv_params and bh_conv_f32_params share
template <class Params>
void SetGeometry(const ConvGeometry& g, Params* p) {
  p->batch = g.batch; p->in_h = g.in_h; p->in_w = g.in_w; p->in_c = g.in_c;
  p->out_h = g.out_h; p->out_w = g.out_w; p->out_c = g.out_c; p->k_h = g.k_h; p->k_w = g.k_w;
  p->stride_h = g.stride_h; p->stride_w = g.stride_w; p->dil_h = g.dil_h; p->dil_w = g.dil_w;
  p->pad_h = g.pad_h; p->pad_w = g.pad_w;
}
// ... and bh_pool_params and bh_pool_f32_params
template <class Params>
void SetGeometry(const PoolGeometry& g, Params* p) {
  p->batch = g.batch; p->in_h = g.in_h; p->in_w = g.in_w; p->channels = g.channels;
  p->out_h = g.out_h; p->out_w = g.out_w; p->f_h = g.f_h; p->f_w = g.f_w;
  p->stride_h = g.stride_h; p->stride_w = g.stride_w; p->pad_h = g.pad_h; p->pad_w = g.pad_w;
}

absl::Status Refused(const TflOperator& op, const char* why) {
  return absl::InternalError(std::string("unsupported ") + TflBuiltinName(op.builtin) + ": " + why);
}

}  // namespace

absl::Status HipModelExecutor::ConstBlob(const std::string& key, size_t bytes, PreparedSubgraph* sg,
                                         const std::function<absl::Status(uint8_t*)>& fill,
                                         std::shared_ptr<DeviceBlob>* out) {
  auto blob = DeviceRegistry::Get().FindConst(ordinal_, key);
  if (!blob) {
    std::vector<uint8_t> host(bytes, 0);
    RETURN_STATUS_IF(fill(host.data()));
    blob = std::make_shared<DeviceBlob>(ordinal_, bytes);
    if (!blob->ok() || !blob->Upload(0, host.data(), bytes)) return HipErr(1, ("upload constant " + key).c_str());
    DeviceRegistry::Get().PutConst(ordinal_, key, blob);
  }
  sg->consts.push_back(blob);
  *out = blob;
  return absl::OkStatus();
}

absl::Status HipModelExecutor::UploadConst(const std::string& key, const void* data, size_t bytes,
                                           PreparedSubgraph* sg, const void** dev) {
  std::shared_ptr<DeviceBlob> blob;
  RETURN_STATUS_IF(ConstBlob(key, bytes, sg, [&](uint8_t* host) {
    if (bytes) std::memcpy(host, data, bytes);
    return absl::OkStatus();
  }, &blob));
  *dev = blob->ptr();
  return absl::OkStatus();
}

absl::Status HipModelExecutor::DevicePtr(const HipModel& model, int t, PreparedSubgraph* sg, void** ptr) {
  const TflTensor& tt = model.desc().tensors[t];
  if (!tt.is_const()) {
    auto it = sg->offset.find(t);
    if (it == sg->offset.end()) return absl::InternalError("tensor without arena slot");
    *ptr = static_cast<char*>(sg->arena->ptr()) + it->second;
    return absl::OkStatus();
  }
  const void* dev = nullptr;
  RETURN_STATUS_IF(UploadConst("m" + Hex(model.serial()) + "/t" + std::to_string(t), tt.data, tt.data_size, sg, &dev));
  *ptr = const_cast<void*>(dev);
  return absl::OkStatus();
}

// The kConv / kConvGrouped launch of geometry g: filters packed with K = kh kw
// icg (one row per output channel) next to the folded bias and the
// multipliers, then the 1x1-GEMV-to-FC rewrite or the residual-ADD fold.
// `flip` packs the filters spatially flipped (TRANSPOSE_CONV).
absl::Status HipModelExecutor::PackedConv(const HipModel& model, int oi, const ConvGeometry& g, bool flip,
                                          const void* in_ptr, void* out_ptr, const std::string& ckey,
                                          PreparedSubgraph* sg, Launch* L) {
  const TflModel& d = model.desc();
  const TflTensor& w = d.tensors[g.filter];
  const TflTensor& out = d.tensors[d.ops[oi].outputs[0]];
  const bool i8 = w.type == DataType::kInt8;
  const ConvQuant q = QuantOf(d, g, out);
  const int oc = g.out_c, kh = g.k_h, kw = g.k_w, icg = g.in_c / g.groups, K = kh * kw * icg;
  int kp = 0, np = 0;
  bh_conv_packed_geometry(oc, K, &kp, &np);
  const size_t wbytes = static_cast<size_t>(kp) * np;
  std::shared_ptr<DeviceBlob> blob;
  RETURN_STATUS_IF(ConstBlob(ckey, wbytes + 12ull * oc, sg, [&](uint8_t* host) {
    std::vector<uint8_t> flipped(flip ? static_cast<size_t>(oc) * K : 0);
    for (size_t i = 0; i < flipped.size(); ++i) {
      const size_t ci = i % icg, fx = i / icg % kw, fy = i / icg / kw % kh, co = i / K;
      flipped[i] = w.data[((co * kh + (kh - 1 - fy)) * kw + (kw - 1 - fx)) * icg + ci];
    }
    int32_t* tables = reinterpret_cast<int32_t*>(host + wbytes);
    if (bh_pack_conv_weights(flip ? flipped.data() : w.data, i8 ? 1 : 0, oc, K, kp, np, q.bias, q.in_zp, q.w_zp,
                             reinterpret_cast<int8_t*>(host), tables) != 0)
      return absl::InternalError("weight packing failed");
    std::copy(q.mult.begin(), q.mult.end(), tables + oc);
    std::copy(q.shift.begin(), q.shift.end(), tables + 2 * oc);
    return absl::OkStatus();
  }, &blob));
  const int32_t* tab = reinterpret_cast<const int32_t*>(static_cast<char*>(blob->ptr()) + wbytes);
  if (g.groups == 1) L->Set<Launch::kConv>();
  else L->Set<Launch::kConvGrouped>({bh_conv_params{}, g.groups});
  bh_conv_params& p = L->conv();
  SetGeometry(g, &p);
  p.k_pad = kp; p.n_pad = np; p.in_xor = i8 ? 0 : 0x80;
  p.in_zp = q.in_zp; p.w_zp = q.w_zp; p.out_zp = Zp(out); p.act_min = q.amin; p.act_max = q.amax;
  p.input = in_ptr; p.output = out_ptr;
  p.weights = static_cast<const int8_t*>(blob->ptr());
  p.bias_eff = tab; p.mult = tab + oc; p.shift = tab + 2 * oc;
  p.requant_fast = bh_conv_requant_fast_ok(q.mult.data(), q.shift.data(), oc, K, MaxAbs(q.bias, oc));
  const double M = static_cast<double>(g.batch) * g.out_h * g.out_w;
  L->alg_ops = 2.0 * M * oc * K;
  L->alg_bytes = static_cast<double>(g.batch) * g.in_h * g.in_w * g.in_c + M * oc + static_cast<double>(oc) * K +
                 12.0 * oc;
  if (g.groups == 1) {
    L->kernel = bh_conv2d_i8_kernel(&p);  // the kernel bh_conv2d_i8 dispatches to
    if (GemvAsFc(L)) return absl::OkStatus();
  } else {
    L->kernel = device_flag_ == DeviceFlag::kCPU ? "conv_grouped_host"
                                                 : bh_conv2d_grouped_i8_kernel(&L->as<bh_conv_grouped_params>());
  }
  TryFuseResidualAdd(model, oi, sg, L);  // the grouped kernel shares the dense epilogue
  return absl::OkStatus();
}

absl::Status HipModelExecutor::LowerConv(const HipModel& model, int oi, void* in_ptr, void* out_ptr,
                                         const std::string& ckey, PreparedSubgraph* sg, Launch* L) {
  ConvGeometry g;
  const char* why = "";
  if (!ConvArgs(model.desc(), model.desc().ops[oi], &g, &why)) return Refused(model.desc().ops[oi], why);
  return PackedConv(model, oi, g, false, in_ptr, out_ptr, ckey, sg, L);
}

// TRANSPOSE_CONV (int8; reference_integer_ops::TransposeConv scatters
// (x - zp) * w into an int32 scratch).  MI355X form: a transpose conv is a
// stride-1 CONV_2D over the zero-inserted input U (U[y*s][x*s] = x, the input
// zero point elsewhere, so inserted positions contribute exactly 0) with
// spatially flipped filters and top/left padding k-1-pad; integer sums are
// order-free, so the result is bit-identical.  Two launches: zero insertion
// into a per-subgraph scratch buffer, then the MFMA conv.
absl::Status HipModelExecutor::LowerTransposeConv(const HipModel& model, int oi, void* out_ptr,
                                                  const std::string& ckey, PreparedSubgraph* sg, Launch* L) {
  const TflModel& d = model.desc();
  ConvGeometry g;
  const char* why = "";
  if (!ConvArgs(d, d.ops[oi], &g, &why)) return Refused(d.ops[oi], why);
  const TflTensor& x = d.tensors[g.input];
  void* x_ptr = nullptr;
  RETURN_STATUS_IF(DevicePtr(model, g.input, sg, &x_ptr));
  const int uh = (g.in_h - 1) * g.stride_h + 1, uw = (g.in_w - 1) * g.stride_w + 1;
  const size_t ubytes = static_cast<size_t>(g.batch) * uh * uw * g.in_c;
  // zero-inserted input in a scratch buffer owned by this subgraph
  auto scratch = std::make_shared<DeviceBlob>(ordinal_, ubytes);
  if (!scratch->ok()) return absl::InternalError("HBM scratch allocation failed");
  sg->consts.push_back(scratch);
  Launch Z;
  Z.op_index = oi;
  Z.kernel = "zero_insert_kernel";
  bh_zero_insert_params& zi = Z.Set<Launch::kZeroInsert>();
  zi.batch = g.batch; zi.in_h = g.in_h; zi.in_w = g.in_w; zi.channels = g.in_c;
  zi.stride_h = g.stride_h; zi.stride_w = g.stride_w; zi.out_h = uh; zi.out_w = uw;
  zi.fill = static_cast<uint32_t>(Zp(x)) & 0xffu;
  zi.input = x_ptr;
  zi.output = scratch->ptr();
  Z.alg_bytes = static_cast<double>(x.num_elements()) + static_cast<double>(ubytes);
  sg->launches.push_back(Z);
  // the stride-1 conv over U: flipped filters, folded bias (int8 filters: zero point 0)
  ConvGeometry u = g;
  u.in_h = uh; u.in_w = uw;
  u.stride_h = u.stride_w = 1;
  u.pad_h = g.k_h - 1 - g.pad_h; u.pad_w = g.k_w - 1 - g.pad_w;
  return PackedConv(model, oi, u, true, scratch->ptr(), out_ptr, ckey, sg, L);
}

// Glue ops.  Every 8-bit unary op becomes a 256-entry
// table built here with TFLite's formula (quant.cc), so the device does a
// byte gather; index maps TFLite computes in float are tabulated here too.
absl::Status HipModelExecutor::LowerGlue(const HipModel& model, int oi, void* in_ptr, void* out_ptr,
                                         const std::string& ckey, PreparedSubgraph* sg, Launch* L) {
  const TflModel& d = model.desc();
  const TflOperator& op = d.ops[oi];
  auto T = [&](int i) -> const TflTensor& { return d.tensors[i]; };
  const TflTensor& in = T(op.inputs[0]);
  const TflTensor& out = T(op.outputs[0]);
  const bool i8 = in.type == DataType::kInt8;
  const double in_bytes = static_cast<double>(meta_[op.inputs[0]]->bytes);
  const double out_bytes = static_cast<double>(meta_[op.outputs[0]]->bytes);
  L->alg_bytes = in_bytes + out_bytes;
  switch (op.builtin) {
    case kTflQuantize:
    case kTflRelu:
    case kTflRelu6:
    case kTflReluN1To1:
    case kTflLogistic:
    case kTflHardSwish:
    case kTflRsqrt:
    case kTflTanh:
    case kTflGelu: {
      const long count = static_cast<long>(out.num_elements());
      if (op.builtin == kTflQuantize && in.type == DataType::kFloat32) {
        L->Set<Launch::kQuantF32>({static_cast<const float*>(in_ptr), out_ptr, count, Scale(out), Zp(out),
                                   out.type == DataType::kInt8 ? 1 : 0});
        L->kernel = "quantize_f32_kernel";
        return absl::OkStatus();
      }
      uint8_t table[256];
      if (op.builtin == kTflQuantize) {
        RequantizeTable(i8, Scale(in), Zp(in), out.type == DataType::kInt8, Scale(out), Zp(out), table);
      } else if (op.builtin == kTflLogistic) {
        LogisticTable(i8, Scale(in), Zp(in), Scale(out), Zp(out), table);
      } else if (op.builtin == kTflHardSwish) {
        if (!HardSwishTable(i8, Scale(in), Zp(in), Scale(out), Zp(out), table))
          return absl::InternalError("HARD_SWISH: output multiplier exponent > 0");
      } else if (op.builtin == kTflRsqrt) {
        if (!RsqrtTable(Scale(in), Zp(in), Scale(out), Zp(out), table))
          return absl::InternalError("RSQRT: output multiplier out of range");
      } else if (op.builtin == kTflTanh) {
        const char* why = "";
        if (!TanhArgs(d, op, nullptr, &why)) return Refused(op, why);
        TanhTable(i8, Scale(in), Zp(in), Scale(out), Zp(out), table);
      } else if (op.builtin == kTflGelu) {
        GeluTable(i8, op.options.valid() && op.options.Bool(0, false), Scale(in), Zp(in), Scale(out), Zp(out), table);
      } else {
        const float lo = op.builtin == kTflReluN1To1 ? -1.0f : 0.0f;
        const float hi = op.builtin == kTflRelu6 ? 6.0f : 1.0f;
        ReluTable(i8, Scale(in), Zp(in), Scale(out), Zp(out), lo, hi, op.builtin == kTflRelu, table);
      }
      LutArgs& a = L->Set<Launch::kLutU8>({in_ptr, out_ptr, count, nullptr});
      RETURN_STATUS_IF(UploadConst(ckey + "/lut", table, sizeof(table), sg, &a.table));
      L->kernel = "lut_u8_kernel";
      return absl::OkStatus();
    }
    case kTflDequantize: {
      float table[256];
      DequantizeTable(i8, Scale(in), Zp(in), table);
      LutArgs& a = L->Set<Launch::kLutF32>({in_ptr, out_ptr, static_cast<long>(out.num_elements()), nullptr});
      RETURN_STATUS_IF(UploadConst(ckey + "/lut", table, sizeof(table), sg, &a.table));
      L->kernel = "lut_f32_kernel";
      return absl::OkStatus();
    }
    case kTflSoftmax: {
      const float beta = op.options.valid() ? op.options.Float(0, 1.0f) : 1.0f;
      float table[256];
      SoftmaxExpTable(Scale(in), beta, table);
      const void* dt = nullptr;
      RETURN_STATUS_IF(UploadConst(ckey + "/exp", table, sizeof(table), sg, &dt));
      bh_softmax_params& p = L->Set<Launch::kSoftmax>();
      p.depth = in.shape.back();
      p.rows = static_cast<long>(in.num_elements() / std::max(p.depth, 1));
      p.is_signed = i8 ? 1 : 0;
      p.table = static_cast<const float*>(dt);
      p.out_scale = Scale(out);
      p.out_zp = Zp(out);
      p.input = in_ptr;
      p.output = out_ptr;
      L->kernel = "softmax_kernel";
      return absl::OkStatus();
    }
    case kTflConcatenation: {
      const int rank = static_cast<int>(out.shape.size());
      int axis = op.options.valid() ? op.options.Int(0, 0) : 0;
      if (axis < 0) axis += rank;
      if (axis < 0 || axis >= rank) return absl::InternalError("CONCATENATION axis out of range");
      long outer = 1, inner = static_cast<long>(GetDataTypeBytes(out.type));
      for (int i = 0; i < axis; ++i) outer *= out.shape[i];
      for (int i = axis + 1; i < rank; ++i) inner *= out.shape[i];
      bh_concat_params& p = L->Set<Launch::kConcat>();
      p.n_inputs = static_cast<int>(op.inputs.size());
      p.outer = outer;
      p.output = out_ptr;
      L->alg_bytes = out_bytes;
      for (int k = 0; k < p.n_inputs; ++k) {
        const TflTensor& x = T(op.inputs[k]);
        void* xp = nullptr;
        RETURN_STATUS_IF(DevicePtr(model, op.inputs[k], sg, &xp));
        p.input[k] = xp;
        p.row[k] = static_cast<long>(x.shape[axis]) * inner;
        L->alg_bytes += static_cast<double>(meta_.size() > static_cast<size_t>(op.inputs[k]) && meta_[op.inputs[k]]
                                                ? meta_[op.inputs[k]]->bytes
                                                : 0);
        if (out.type == DataType::kUInt8 && (Zp(x) != Zp(out) || Scale(x) != Scale(out))) {
          uint8_t table[256];
          ConcatRescaleTable(Scale(x), Zp(x), Scale(out), Zp(out), table);
          RETURN_STATUS_IF(UploadConst(ckey + "/lut" + std::to_string(k), table, sizeof(table), sg, &p.table[k]));
        }
      }
      L->kernel = "concat_kernel";
      return absl::OkStatus();
    }
    case kTflPack: {
      // np.stack is a concatenation of the inputs' remainders past the axis
      bh_concat_params& p = L->Set<Launch::kConcat>();
      const char* why = "";
      if (!PackArgs(d, op, &p, &why)) return Refused(op, why);
      p.output = out_ptr;
      for (int k = 0; k < p.n_inputs; ++k) {
        void* xp = nullptr;
        RETURN_STATUS_IF(DevicePtr(model, op.inputs[k], sg, &xp));
        p.input[k] = xp;
      }
      L->alg_bytes = 2.0 * out_bytes;
      L->kernel = "concat_kernel";
      return absl::OkStatus();
    }
    case kTflPad:
    case kTflPadV2:
    case kTflMirrorPad: {
      const int rank = static_cast<int>(in.shape.size());
      std::vector<int64_t> pads(2 * static_cast<size_t>(rank), 0);
      int mirror = 0;
      if (op.builtin == kTflMirrorPad && !MirrorPadArgs(d, op, &pads, &mirror))
        return absl::InternalError("MIRROR_PAD arguments");
      std::vector<int64_t> given;
      if (!mirror && ConstInts(T(op.inputs[1]), &given))  // PAD / PADV2
        std::copy_n(given.begin(), std::min(given.size(), pads.size()), pads.begin());
      bh_pad_params& p = L->Set<Launch::kPad>();
      p.elem_bytes = static_cast<int>(GetDataTypeBytes(in.type));
      Shape4(in.shape, p.in_shape);
      const int lead = 4 - rank;
      for (int dd = 0; dd < rank; ++dd) {
        p.pad_before[lead + dd] = static_cast<int>(pads[2 * dd]);
        p.pad_after[lead + dd] = static_cast<int>(pads[2 * dd + 1]);
      }
      uint32_t value = 0;
      if (op.builtin == kTflPadV2 && op.inputs.size() > 2 && op.inputs[2] >= 0) {
        const TflTensor& cv = T(op.inputs[2]);
        std::memcpy(&value, cv.data, std::min<size_t>(cv.data_size, p.elem_bytes));
      } else if (IsQ8(in.type)) {
        value = static_cast<uint32_t>(Zp(out)) & 0xffu;  // quantized PAD pads with the output zero point
      }
      p.value = value;
      p.mode = mirror;
      p.input = in_ptr;
      p.output = out_ptr;
      L->kernel = "pad_kernel";
      return absl::OkStatus();
    }
    case kTflResizeNearestNeighbor:
    case kTflResizeBilinear: {
      const int b = in.shape[0], ih = in.shape[1], iw = in.shape[2], c = in.shape[3];
      const int oh = out.shape[1], ow = out.shape[2];
      const bool nearest = op.builtin == kTflResizeNearestNeighbor;
      const bool ac = op.options.valid() && op.options.Bool(nearest ? 0 : 2, false);
      const bool hp = op.options.valid() && op.options.Bool(nearest ? 1 : 3, false);
      if (nearest) {
        std::vector<int32_t> tab(static_cast<size_t>(oh) + ow);
        for (int y = 0; y < oh; ++y) tab[y] = NearestNeighborIndex(y, ih, oh, ac, hp);
        for (int x = 0; x < ow; ++x) tab[oh + x] = NearestNeighborIndex(x, iw, ow, ac, hp);
        const void* dt = nullptr;
        RETURN_STATUS_IF(UploadConst(ckey + "/idx", tab.data(), tab.size() * 4, sg, &dt));
        bh_resize_nearest_params& p = L->Set<Launch::kResizeNearest>();
        p.batch = b; p.in_h = ih; p.in_w = iw; p.out_h = oh; p.out_w = ow;
        p.row_bytes = c * static_cast<int>(GetDataTypeBytes(in.type));
        p.y_index = static_cast<const int32_t*>(dt);
        p.x_index = static_cast<const int32_t*>(dt) + oh;
        p.input = in_ptr;
        p.output = out_ptr;
        L->kernel = "resize_nearest_kernel";
      } else if (in.type == DataType::kUInt8) {
        // uint8: optimized_ops::ResizeBilinear's float path
        std::vector<int32_t> iy, ix;
        std::vector<float> fy, fx;
        BilinearFloatTable(ih, oh, ac, hp, &iy, &fy);
        BilinearFloatTable(iw, ow, ac, hp, &ix, &fx);
        // one upload: {y_idx, x_idx} int32 then {y_frac, x_frac} float
        std::vector<int32_t> blob(iy);
        blob.insert(blob.end(), ix.begin(), ix.end());
        blob.resize(blob.size() + fy.size() + fx.size());
        std::memcpy(blob.data() + iy.size() + ix.size(), fy.data(), fy.size() * 4);
        std::memcpy(blob.data() + iy.size() + ix.size() + fy.size(), fx.data(), fx.size() * 4);
        const void* dt = nullptr;
        RETURN_STATUS_IF(UploadConst(ckey + "/tab8", blob.data(), blob.size() * 4, sg, &dt));
        const int32_t* t32 = static_cast<const int32_t*>(dt);
        bh_resize_bilinear_u8_params& p = L->Set<Launch::kResizeBilinearU8>();
        p.batch = b; p.in_h = ih; p.in_w = iw; p.channels = c; p.out_h = oh; p.out_w = ow;
        p.y_idx = t32;
        p.x_idx = t32 + 2 * oh;
        p.y_frac = reinterpret_cast<const float*>(t32 + 2 * oh + 2 * ow);
        p.x_frac = reinterpret_cast<const float*>(t32 + 3 * oh + 2 * ow);
        p.input = in_ptr;
        p.output = out_ptr;
        L->kernel = "resize_bilinear_u8_kernel";
      } else {
        std::vector<int32_t> ty, tx;
        BilinearIntegerTable(ih, oh, ac, hp, &ty);
        BilinearIntegerTable(iw, ow, ac, hp, &tx);
        ty.insert(ty.end(), tx.begin(), tx.end());
        const void* dt = nullptr;
        RETURN_STATUS_IF(UploadConst(ckey + "/tab", ty.data(), ty.size() * 4, sg, &dt));
        bh_resize_bilinear_params& p = L->Set<Launch::kResizeBilinear>();
        p.batch = b; p.in_h = ih; p.in_w = iw; p.channels = c; p.out_h = oh; p.out_w = ow;
        p.y_tab = static_cast<const int32_t*>(dt);
        p.x_tab = static_cast<const int32_t*>(dt) + 3 * oh;
        p.input = in_ptr;
        p.output = out_ptr;
        L->kernel = "resize_bilinear_kernel";  // (row forms resize_bilinear_rows_kernel / resize_bilinear_cols_kernel when the rows fit LDS)
      }
      return absl::OkStatus();
    }
    default:
      return absl::InternalError(std::string("no lowering for ") + TflBuiltinName(op.builtin));
  }
}

absl::Status HipModelExecutor::BuildLaunches(const HipModel& model, PreparedSubgraph* sg) {
  sg->launches.clear();
  sg->fused_ops.clear();
  sg->fused_tensors.clear();
  for (int i : sg->ops) {
    if (sg->fused_ops.count(i)) continue;
    RETURN_STATUS_IF(Lower(model, i, sg));
  }
  // fused chains / blocks are GPU kernels picked by on-device timing; chains
  // first (they cut more launches), blocks over what the chains left
  if (opt_.allow_fusion && opt_.allow_chain && device_flag_ == DeviceFlag::kGPU) FuseChains(model, sg);
  if (opt_.allow_fusion && opt_.allow_irb && device_flag_ == DeviceFlag::kGPU) FuseBlocks(model, sg);
  if (opt_.allow_fusion && opt_.allow_layernorm && device_flag_ == DeviceFlag::kGPU) FuseLayerNorm(model, sg);
  if (opt_.allow_fusion && opt_.allow_layernorm && opt_.fused_layernorm_f32 && device_flag_ == DeviceFlag::kGPU) {
    FuseLayerNormF32(model, sg);
    FoldLayerNormQuant(model, sg);
  }
  if (opt_.allow_fusion && opt_.fused_attention && device_flag_ == DeviceFlag::kGPU) FuseAttention(model, sg);
  if (opt_.allow_fusion) FuseGlue(model, sg);
  if (opt_.allow_fusion && opt_.allow_group && device_flag_ == DeviceFlag::kGPU) RETURN_STATUS_IF(GroupConvs(sg));
  return absl::OkStatus();
}

// Folds `conv -> ADD/SUB(conv_out, residual)` into the conv epilogue when the
// conv output has no other reader and nobody needs it materialised.  The
// epilogue reproduces both TFLite ops exactly (conv requant + clamp to the
// conv's 8-bit output, then add.cc's arithmetic), so the result is
// bit-identical to running the two ops.
bool HipModelExecutor::TryFuseResidualAdd(const HipModel& model, int oi, PreparedSubgraph* sg, Launch* L) {
  if (!opt_.allow_fusion || !opt_.allow_add) return false;
  const TflModel& d = model.desc();
  const int t = d.ops[oi].outputs[0];
  if (consumers_[t].size() != 1) return false;
  const int j = consumers_[t][0];
  if (j <= oi || !std::binary_search(sg->ops.begin(), sg->ops.end(), j)) return false;
  const TflOperator& add = d.ops[j];
  if ((add.builtin != kTflAdd && add.builtin != kTflSub) || add.inputs.size() != 2) return false;
  if (!GpuSupports(d, add, nullptr)) return false;
  if (KeptOutside(d, *sg, t)) return false;
  const bool conv_is_first = add.inputs[0] == t;
  const int other = conv_is_first ? add.inputs[1] : add.inputs[0];
  if (other == t) return false;
  // the epilogue reads the other operand while the conv runs, so it must
  // already exist then: produced by an earlier op (an FPN's ADD of a lateral
  // conv and an upsampled map produced later must stay unfused)
  if (other < 0 || producer_[other] > oi) return false;
  const TflTensor& tc = d.tensors[t];
  const TflTensor& tr = d.tensors[other];
  const TflTensor& to = d.tensors[add.outputs[0]];
  if (tr.shape != tc.shape || to.shape != tc.shape || tr.type != tc.type || to.type != tc.type) return false;
  void* rptr = nullptr;
  void* optr = nullptr;
  if (!DevicePtr(model, other, sg, &rptr).ok() || !DevicePtr(model, add.outputs[0], sg, &optr).ok()) return false;
  const TflTensor& t1 = d.tensors[add.inputs[0]];
  const TflTensor& t2 = d.tensors[add.inputs[1]];
  const AddParams ap = AddSubParams(Scale(t1), Scale(t2), Scale(to), add.builtin == kTflSub);
  bh_conv_params& p = L->conv();
  p.residual = rptr;
  p.output = optr;
  p.add_left_shift = ap.left_shift;
  p.add_y_off = -Zp(tc);
  p.add_r_off = -Zp(tr);
  p.add_o_off = Zp(to);
  p.add_y_mult = conv_is_first ? ap.m1 : ap.m2;
  p.add_y_shift = conv_is_first ? ap.s1 : ap.s2;
  p.add_r_mult = conv_is_first ? ap.m2 : ap.m1;
  p.add_r_shift = conv_is_first ? ap.s2 : ap.s1;
  p.add_o_mult = ap.mo;
  p.add_o_shift = ap.so;
  const int act = add.options.valid() ? add.options.Int8(0, 0) : 0;
  ActivationRangeQuantized(act, Scale(to), Zp(to), to.type == DataType::kInt8, &p.add_act_min, &p.add_act_max);
  L->alg_bytes += static_cast<double>(tr.num_elements());  // residual read; y never stored
  L->kernel = WithAdd(L->kernel);
  sg->fused_ops.insert(j);
  L->out_tensor = add.outputs[0];
  sg->fused_tensors.insert(t);
  return true;
}

// float32 graphs (fp16-weight models): constants (fp16 behind DEQUANTIZE,
// or float32) are folded on the host into the layouts the bh_*_f32 kernels
// read; a DEQUANTIZE whose consumers all fold it emits nothing.
absl::Status HipModelExecutor::LowerFloat(const HipModel& model, int oi, void* in_ptr, void* out_ptr,
                                          const std::string& ckey, PreparedSubgraph* sg, Launch* L, bool* emit) {
  const TflModel& d = model.desc();
  const TflOperator& op = d.ops[oi];
  auto T = [&](int i) -> const TflTensor& { return d.tensors[i]; };
  const TflTensor& in = T(op.inputs[0]);
  const TflTensor& out = T(op.outputs[0]);
  const double io_bytes = 4.0 * (static_cast<double>(in.num_elements()) + out.num_elements());
  L->alg_bytes = io_bytes;
  auto upload = [&](const std::string& key, const std::vector<float>& v, const float** dev) {
    return UploadConst(key, v.data(), v.size() * sizeof(float), sg, reinterpret_cast<const void**>(dev));
  };
  const char* why = "";
  switch (op.builtin) {
    case kTflDequantize: {
      const int t = op.outputs[0];
      bool all_fold = true;
      for (int c : consumers_[t]) {
        const TflOperator& co = d.ops[c];
        const bool folds = (co.builtin == kTflConv2D || co.builtin == kTflDepthwiseConv2D ||
                            co.builtin == kTflFullyConnected) &&
                           co.inputs[0] != t;
        all_fold = all_fold && folds;
      }
      if (all_fold && !KeptOutside(d, *sg, t)) {
        sg->fused_tensors.insert(t);  // never materialised: a view of it re-lowers with the copy
        *emit = false;
        return absl::OkStatus();
      }
      const float* dev = nullptr;
      RETURN_STATUS_IF(upload(ckey + "/f32", FloatData(d, t), &dev));
      const CopyArgs& c = L->Set<Launch::kCopy>({out_ptr, dev, 4 * out.num_elements()});
      L->kernel = "copy";
      L->alg_bytes = 2.0 * c.bytes;
      return absl::OkStatus();
    }
    case kTflConv2D:
    case kTflDepthwiseConv2D: {
      if (opt_.hybrid_conv && IsHybridConvOp(d, op)) return LowerConvHybrid(model, oi, in_ptr, out_ptr, ckey, sg, L);
      const bool dw = op.builtin == kTflDepthwiseConv2D;
      ConvGeometry g;
      if (!ConvArgs(d, op, &g, &why)) return Refused(op, why);
      const int oc = g.out_c;
      std::vector<float> wf = FloatData(d, g.filter);
      std::vector<float> laid(wf.size());
      if (dw) {
        laid = wf;  // [1][kh][kw][oc] is already [kh*kw][oc]
      } else {
        const int K = g.k_h * g.k_w * g.in_c;  // OHWI -> [K][oc]
        for (int c = 0; c < oc; ++c)
          for (int k = 0; k < K; ++k) laid[static_cast<size_t>(k) * oc + c] = wf[static_cast<size_t>(c) * K + k];
      }
      bh_conv_f32_params& p = L->Set<Launch::kConvF32>();
      RETURN_STATUS_IF(upload(ckey + "/w", laid, &p.weights));
      if (g.bias >= 0) RETURN_STATUS_IF(upload(ckey + "/b", FloatData(d, g.bias), &p.bias));
      SetGeometry(g, &p);
      p.depthwise = dw ? 1 : 0;
      p.depth_multiplier = g.depth_multiplier;
      FloatActRange(g.act, &p.act_min, &p.act_max);
      p.input = static_cast<const float*>(in_ptr);
      p.output = static_cast<float*>(out_ptr);
      L->kernel = dw ? "dwconv_f32_kernel" : "conv_f32_kernel";
      L->alg_ops = 2.0 * g.batch * g.out_h * g.out_w * oc * g.k_h * g.k_w * (dw ? 1 : g.in_c);
      L->alg_bytes = io_bytes + 4.0 * laid.size() + 4.0 * oc;
      return absl::OkStatus();
    }
    case kTflFullyConnected: {
      if (IsHybridWeightOp(d, op)) return LowerFcHybrid(model, oi, in_ptr, out_ptr, ckey, sg, L);
      FcGeometry g;
      if (!FcArgs(d, op, &g, &why)) return Refused(op, why);
      bh_fc_f32_params& p = L->Set<Launch::kFcF32>();
      RETURN_STATUS_IF(upload(ckey + "/w", FloatData(d, g.filter), &p.weights));
      if (g.bias >= 0) RETURN_STATUS_IF(upload(ckey + "/b", FloatData(d, g.bias), &p.bias));
      p.rows = g.rows;
      p.depth = g.depth;
      p.units = g.units;
      FloatActRange(g.act, &p.act_min, &p.act_max);
      p.input = static_cast<const float*>(in_ptr);
      p.output = static_cast<float*>(out_ptr);
      L->kernel = "fc_f32_kernel";
      L->alg_ops = 2.0 * p.rows * g.units * g.depth;
      L->alg_bytes = io_bytes + 4.0 * g.units * g.depth;
      return absl::OkStatus();
    }
    case kTflAdd:
    case kTflSub:
    case kTflMul:
    case kTflSquaredDifference: {
      BroadcastShapes s;
      if (!BroadcastArgs(d, op, &s, &why)) return Refused(op, why);
      void* b_ptr = nullptr;
      RETURN_STATUS_IF(DevicePtr(model, op.inputs[1], sg, &b_ptr));
      bh_eltwise_f32_params& p = L->Set<Launch::kEltwiseF32>();
      p.kind = op.builtin == kTflAdd   ? BH_ELTF_ADD
               : op.builtin == kTflSub ? BH_ELTF_SUB
               : op.builtin == kTflMul ? BH_ELTF_MUL
                                       : BH_ELTF_SQDIFF;
      std::copy_n(s.a, 4, p.shape_a); std::copy_n(s.b, 4, p.shape_b); std::copy_n(s.o, 4, p.shape_o);
      FloatActRange(op.options.Int8(0, 0), &p.act_min, &p.act_max);
      p.a = static_cast<const float*>(in_ptr);
      p.b = static_cast<const float*>(b_ptr);
      p.out = static_cast<float*>(out_ptr);
      L->kernel = "eltwise_f32_kernel";
      L->alg_bytes += 4.0 * T(op.inputs[1]).num_elements();
      return absl::OkStatus();
    }
    case kTflAveragePool2D:
    case kTflMaxPool2D: {
      PoolGeometry g;
      if (!PoolArgs(d, op, &g, &why)) return Refused(op, why);
      bh_pool_f32_params& p = L->Set<Launch::kPoolF32>();
      p.kind = op.builtin == kTflAveragePool2D ? BH_POOL_AVG : BH_POOL_MAX;
      SetGeometry(g, &p);
      FloatActRange(g.act, &p.act_min, &p.act_max);
      p.input = static_cast<const float*>(in_ptr);
      p.output = static_cast<float*>(out_ptr);
      L->kernel = "pool_f32_kernel";
      return absl::OkStatus();
    }
    case kTflSoftmax: {
      const int depth = in.shape.back();
      L->Set<Launch::kSoftmaxF32>({static_cast<const float*>(in_ptr), static_cast<float*>(out_ptr),
                                   static_cast<long>(in.num_elements() / std::max(depth, 1)), depth,
                                   op.options.valid() ? op.options.Float(0, 1.0f) : 1.0f});
      L->kernel = "softmax_f32_kernel";
      return absl::OkStatus();
    }
    case kTflBatchMatMul:
      return LowerBatchMatMul(model, oi, in_ptr, out_ptr, sg, L);
    default: {  // RELU / RELU6 / RELU_N1_TO_1 / LOGISTIC / RSQRT / GELU / TANH
      UnaryF32Args& a = L->Set<Launch::kUnaryF32>();
      L->kernel = "unary_f32_kernel";
      const bool approximate = op.builtin == kTflGelu && op.options.valid() && op.options.Bool(0, false);
      a.kind = op.builtin == kTflLogistic ? BH_UNARY_LOGISTIC
               : op.builtin == kTflTanh   ? BH_UNARY_TANH
               : op.builtin == kTflRsqrt  ? BH_UNARY_RSQRT
               : op.builtin == kTflGelu   ? (approximate ? BH_UNARY_GELU_TANH : BH_UNARY_GELU)
                                          : BH_UNARY_CLAMP;
      a.lo = op.builtin == kTflReluN1To1 ? -1.f : 0.f;
      a.hi = op.builtin == kTflRelu6 ? 6.f : (op.builtin == kTflReluN1To1 ? 1.f : std::numeric_limits<float>::infinity());
      a.count = static_cast<long>(in.num_elements());
      a.src = static_cast<const float*>(in_ptr);
      a.dst = static_cast<float*>(out_ptr);
      return absl::OkStatus();
    }
  }
}

bool HipModelExecutor::DequantFoldsIntoDetection(const TflModel& d, const PreparedSubgraph& sg, int oi) const {
  if (device_flag_ != DeviceFlag::kGPU || !opt_.gpu_detection || !opt_.allow_fusion) return false;
  const TflOperator& op = d.ops[oi];
  if (op.builtin != kTflDequantize || op.inputs.empty() || op.inputs[0] < 0 || op.outputs.empty()) return false;
  const TflTensor& in = d.tensors[op.inputs[0]];
  const int t = op.outputs[0];
  // the byte maximum is the float maximum only for an increasing dequantisation
  if (t < 0 || !IsQ8(in.type) || !HasQ(in) || !(Scale(in) > 0.0f) || d.tensors[t].type != DataType::kFloat32)
    return false;
  if (consumers_[t].size() != 1) return false;
  const int j = consumers_[t][0];
  if (!std::binary_search(sg.ops.begin(), sg.ops.end(), j)) return false;
  int batch = 1;
  const TflOperator& det = d.ops[j];
  if (!DetectionSupported(d, det, nullptr, &batch) || (det.inputs[0] != t && det.inputs[1] != t)) return false;
  return !KeptOutside(d, sg, t);
}

absl::Status HipModelExecutor::LowerDetectionGpu(const HipModel& model, int oi, PreparedSubgraph* sg, Launch* L) {
  const TflModel& d = model.desc();
  const TflOperator& op = d.ops[oi];
  CpuDetectionParams c{};
  int batch = 1;
  if (!opt_.gpu_detection || !DetectionSupported(d, op, &c, &batch))
    return absl::InternalError("unsupported custom op " + op.custom_code);
  bh_detection_params& p = L->Set<Launch::kDetectionGpu>();
  p.batch = batch;
  p.num_boxes = c.num_boxes;
  p.num_classes = c.num_classes;
  p.num_classes_with_background = c.num_classes_with_background;
  p.max_detections = c.max_detections;
  p.score_threshold = c.score_threshold;
  p.iou_threshold = c.iou_threshold;
  p.scale_y = c.scale_y; p.scale_x = c.scale_x; p.scale_h = c.scale_h; p.scale_w = c.scale_w;
  double bytes = 0;
  // box encodings / class scores: the float tensor, or the 8-bit input of
  // the DEQUANTIZE that produces it when that op was folded away
  auto source = [&](int t, int* type, float* scale, int32_t* zp, const void** ptr) -> absl::Status {
    int src = t;
    const int prod = producer_[t];
    if (prod >= 0 && DequantFoldsIntoDetection(d, *sg, prod)) {
      src = d.ops[prod].inputs[0];
      const TflTensor& q = d.tensors[src];
      *type = q.type == DataType::kInt8 ? 1 : 2;
      *scale = Scale(q);
      *zp = Zp(q);
    }
    void* dev = nullptr;
    RETURN_STATUS_IF(DevicePtr(model, src, sg, &dev));
    *ptr = dev;
    bytes += static_cast<double>(meta_[src]->bytes);
    return absl::OkStatus();
  };
  RETURN_STATUS_IF(source(op.inputs[0], &p.box_type, &p.box_scale, &p.box_zp, &p.box_encodings));
  RETURN_STATUS_IF(source(op.inputs[1], &p.score_type, &p.score_scale, &p.score_zp, &p.class_scores));
  void* anchors = nullptr;
  void* outs[4];
  RETURN_STATUS_IF(DevicePtr(model, op.inputs[2], sg, &anchors));
  for (int k = 0; k < 4; ++k) {
    RETURN_STATUS_IF(DevicePtr(model, op.outputs[k], sg, &outs[k]));
    bytes += static_cast<double>(meta_[op.outputs[k]]->bytes);
  }
  bytes += 16.0 * c.num_boxes;
  p.anchors = static_cast<const float*>(anchors);
  p.out_boxes = static_cast<float*>(outs[0]);
  p.out_classes = static_cast<float*>(outs[1]);
  p.out_scores = static_cast<float*>(outs[2]);
  p.out_num = static_cast<float*>(outs[3]);
  // the kernels' scratch, sized here and owned by the subgraph; every pass
  // rewrites what it reads of it
  auto scratch = std::make_shared<DeviceBlob>(ordinal_, bh_detection_scratch_bytes(batch, c.num_boxes));
  if (!scratch->ok()) return absl::InternalError("HBM scratch allocation failed");
  sg->consts.push_back(scratch);
  p.scratch = scratch->ptr();
  L->kernel = "detection_postprocess_kernel";
  L->alg_bytes = bytes;
  return absl::OkStatus();
}

// TRANSPOSE / STRIDED_SLICE / SLICE / SPLIT / SPLIT_V / SPACE_TO_DEPTH /
// DEPTH_TO_SPACE / UNPACK / TILE: each output is one map (ReindexArgs) and one
// launch - a SPLIT or an UNPACK with n outputs is n launches, each writing its
// own dense tensor.
absl::Status HipModelExecutor::LowerReindex(const HipModel& model, int oi, PreparedSubgraph* sg) {
  const TflModel& d = model.desc();
  const TflOperator& op = d.ops[oi];
  void* in_ptr = nullptr;
  RETURN_STATUS_IF(DevicePtr(model, op.inputs[op.builtin == kTflSplit ? 1 : 0], sg, &in_ptr));
  for (int k = 0; k < static_cast<int>(op.outputs.size()); ++k) {
    Launch L;
    L.op_index = oi;
    L.out_tensor = op.outputs[k];
    const char* why = "";
    bh_reindex_params& r = L.Set<Launch::kReindex>();
    if (!ReindexArgs(d, op, k, &r, &why))
      return absl::InternalError(std::string("unsupported ") + TflBuiltinName(op.builtin) + ": " + why);
    void* out_ptr = nullptr;
    RETURN_STATUS_IF(DevicePtr(model, op.outputs[k], sg, &out_ptr));
    r.input = in_ptr;
    r.output = out_ptr;
    bh_reindex_params c;
    if (bh_reindex_canonical(&r, &c) != 0)
      return absl::InternalError(std::string(TflBuiltinName(op.builtin)) + ": " + bh_last_error());
    const size_t bytes = meta_[op.outputs[k]]->bytes;
    L.alg_bytes = 2.0 * bytes;
    if (c.rank == 1 && c.in_stride[0] == 1 && c.in_offset == 0) {
      // the identity (a TRANSPOSE that only moves unit dims, a SLICE of
      // everything): same bytes, as RESHAPE
      if (in_ptr == out_ptr) continue;
      L.Set<Launch::kCopy>({out_ptr, in_ptr, bytes});
      L.kernel = "copy";
    } else {
      L.kernel = device_flag_ == DeviceFlag::kCPU ? "reindex_host" : bh_reindex_kernel(&r);
    }
    sg->launches.push_back(L);
  }
  return absl::OkStatus();
}

// GATHER: one kReindex launch whose map carries the index tensor - [outer]
// [n_idx][inner] over GatherArgs' counts - so bh_reindex / CpuReindex hand it
// to bh_gather / CpuGather.  A constant params (an embedding table) and a
// constant indices tensor are uploaded once per (model, GPU), as a filter is;
// a runtime indices tensor is read from its arena slot (a model input lands
// there like any other).  With outer == 1 and the constant indices 0 ..
// axis_size - 1 the output is params byte for byte: a copy, as LowerReindex
// makes of the identity.  The launch joins no fusion pattern (the head
// TRANSPOSE matchers ask for a TRANSPOSE op).
absl::Status HipModelExecutor::LowerGather(const HipModel& model, int oi, PreparedSubgraph* sg) {
  const TflModel& d = model.desc();
  const TflOperator& op = d.ops[oi];
  Launch L;
  L.op_index = oi;
  L.out_tensor = op.outputs[0];
  bh_gather_params p;
  const char* why = "";
  const bool lookup = op.builtin == kTflEmbeddingLookup;  // (ids, table): the operands exchanged, axis 0
  if (!(lookup ? EmbeddingLookupArgs(d, op, &p, &why) : GatherArgs(d, op, &p, &why))) return Refused(op, why);
  int pi = 0, ii = 1;
  GatherOperands(op, &pi, &ii);
  void* params = nullptr;
  void* indices = nullptr;
  void* out_ptr = nullptr;
  RETURN_STATUS_IF(DevicePtr(model, op.inputs[pi], sg, &params));
  RETURN_STATUS_IF(DevicePtr(model, op.inputs[ii], sg, &indices));
  RETURN_STATUS_IF(DevicePtr(model, op.outputs[0], sg, &out_ptr));
  p.params = params;
  p.indices = indices;
  p.output = out_ptr;
  if (bh_gather_check(&p) != 0) return absl::InternalError(std::string("GATHER: ") + bh_last_error());
  const size_t bytes = meta_[op.outputs[0]]->bytes;
  std::vector<int64_t> idx;
  bool identity = p.outer == 1 && p.n_idx == p.axis_size && ConstInts(d.tensors[op.inputs[ii]], &idx);
  for (size_t i = 0; identity && i < idx.size(); ++i) identity = idx[i] == static_cast<int64_t>(i);
  if (identity) {
    if (params == out_ptr) return absl::OkStatus();
    L.Set<Launch::kCopy>({out_ptr, params, bytes});
    L.kernel = "copy";
    L.alg_bytes = 2.0 * bytes;
  } else {
    // (bh_gather_check: every count fits an int)
    bh_reindex_params& r = L.Set<Launch::kReindex>();
    r.elem_bytes = p.elem_bytes;
    r.rank = 3;
    r.out_dims[0] = static_cast<int>(p.outer);
    r.out_dims[1] = static_cast<int>(p.n_idx);
    r.out_dims[2] = static_cast<int>(p.inner);
    r.in_stride[0] = p.axis_size * p.inner;
    r.in_stride[1] = p.inner;
    r.in_stride[2] = 1;
    r.input = params;
    r.output = out_ptr;
    r.indices = indices;
    r.index_bytes = p.index_bytes;
    r.index_range = p.axis_size;
    L.kernel = device_flag_ == DeviceFlag::kCPU ? "gather_host" : bh_reindex_kernel(&r);
    L.alg_bytes = 2.0 * bytes + static_cast<double>(p.n_idx * p.index_bytes);
  }
  sg->launches.push_back(L);
  return absl::OkStatus();
}

// BATCH_MATMUL (int8 / float32): one launch over BatchMatMulArgs' stride form.
// Both operands may be activations; a constant one is uploaded as it is (no
// repacking).  The launch joins no chain, block or conv group and takes no
// epilogue fold.
absl::Status HipModelExecutor::LowerBatchMatMul(const HipModel& model, int oi, void* lhs_ptr, void* out_ptr,
                                                PreparedSubgraph* sg, Launch* L) {
  const TflModel& d = model.desc();
  const TflOperator& op = d.ops[oi];
  const char* why = "";
  const bool f32 = d.tensors[op.inputs[0]].type == DataType::kFloat32;
  bh_batch_matmul_params& p = L->Set(f32 ? Launch::kBatchMatMulF32 : Launch::kBatchMatMul, bh_batch_matmul_params{});
  if (!BatchMatMulArgs(d, op, &p, &why)) return absl::InternalError(std::string("unsupported BATCH_MATMUL: ") + why);
  void* rhs_ptr = nullptr;
  RETURN_STATUS_IF(DevicePtr(model, op.inputs[1], sg, &rhs_ptr));
  p.lhs = lhs_ptr;
  p.rhs = rhs_ptr;
  p.out = out_ptr;
  if (bh_batch_matmul_check(&p, f32 ? 4 : 1) != 0) return absl::InternalError(std::string("BATCH_MATMUL: ") + bh_last_error());
  const bool cpu = device_flag_ == DeviceFlag::kCPU;
  L->kernel = f32 ? (cpu ? "batch_matmul_f32_host" : "bmm_f32_kernel")
                  : (cpu ? "batch_matmul_host" : bh_batch_matmul_i8_kernel(&p));
  L->alg_ops = 2.0 * p.batch[0] * p.batch[1] * p.m * p.n * p.k;
  // operands and output once each; a broadcast operand holds fewer bytes than the batch reads
  L->alg_bytes = static_cast<double>(meta_[op.inputs[0]]->bytes + meta_[op.outputs[0]]->bytes) +
                 static_cast<double>(GetDataTypeBytes(d.tensors[op.inputs[1]].type) * d.tensors[op.inputs[1]].num_elements());
  return absl::OkStatus();
}

absl::Status HipModelExecutor::LowerDepthwise(const HipModel& model, int oi, void* in_ptr, void* out_ptr,
                                              const std::string& ckey, PreparedSubgraph* sg, Launch* L) {
  const TflModel& d = model.desc();
  const TflOperator& op = d.ops[oi];
  ConvGeometry g;
  const char* why = "";
  if (!ConvArgs(d, op, &g, &why)) return Refused(op, why);
  const TflTensor& in = d.tensors[g.input];
  const TflTensor& w = d.tensors[g.filter];
  const TflTensor& out = d.tensors[op.outputs[0]];
  const bool i8 = in.type == DataType::kInt8;
  const ConvQuant q = QuantOf(d, g, out);
  const int oc = g.out_c, kh = g.k_h, kw = g.k_w;
  const size_t wbytes = static_cast<size_t>(kh) * kw * oc;
  const size_t wpad = (wbytes + 15) / 16 * 16;
  const size_t tbytes = 12ull * oc;
  // 3x3 / dm 1 layers also get the dot4 kernel's tap table (bh_pack_dw_taps)
  const bool dot = kh == 3 && kw == 3 && g.depth_multiplier == 1 && oc % 4 == 0;
  const size_t pbytes = dot ? 16ull * oc : 0;
  std::shared_ptr<DeviceBlob> blob;
  RETURN_STATUS_IF(ConstBlob(ckey, wpad + tbytes + pbytes, sg, [&](uint8_t* host) {
    for (size_t i = 0; i < wbytes; ++i) host[i] = i8 ? w.data[i] : static_cast<uint8_t>(w.data[i] ^ 0x80);
    int32_t* tables = reinterpret_cast<int32_t*>(host + wpad);
    for (int c = 0; c < oc; ++c) tables[c] = q.bias ? q.bias[c] : 0;
    std::copy(q.mult.begin(), q.mult.end(), tables + oc);
    std::copy(q.shift.begin(), q.shift.end(), tables + 2 * oc);
    if (dot && bh_pack_dw_taps(reinterpret_cast<const int8_t*>(host), oc, tables, q.in_zp, q.w_zp, tables + 3 * oc) != 0)
      return absl::InternalError("depthwise tap packing failed");
    return absl::OkStatus();
  }, &blob));
  const int32_t* tab = reinterpret_cast<const int32_t*>(static_cast<char*>(blob->ptr()) + wpad);
  bh_dwconv_params& p = L->Set<Launch::kDwConv>();
  SetGeometry(g, &p);
  p.depth_multiplier = g.depth_multiplier;
  p.in_xor = i8 ? 0 : 0x80; p.in_zp = q.in_zp; p.w_zp = q.w_zp; p.out_zp = Zp(out);
  p.act_min = q.amin; p.act_max = q.amax; p.input = in_ptr; p.output = out_ptr;
  p.weights = static_cast<const int8_t*>(blob->ptr());
  p.bias = tab; p.mult = tab + oc; p.shift = tab + 2 * oc;
  if (dot && !blob->host()) p.taps = tab + 3 * oc;
  p.requant_fast = bh_conv_requant_fast_ok(q.mult.data(), q.shift.data(), oc, kh * kw, MaxAbs(q.bias, oc));
  L->kernel = bh_dwconv2d_i8_kernel(&p);  // the kernel bh_dwconv2d_i8 dispatches to
  const double M = static_cast<double>(g.batch) * g.out_h * g.out_w;
  L->alg_ops = 2.0 * M * oc * kh * kw;
  L->alg_bytes = static_cast<double>(in.num_elements()) + M * oc + static_cast<double>(wbytes) + 12.0 * oc;
  return absl::OkStatus();
}

absl::Status HipModelExecutor::LowerFc(const HipModel& model, int oi, void* in_ptr, void* out_ptr,
                                       const std::string& ckey, PreparedSubgraph* sg, Launch* L) {
  const TflModel& d = model.desc();
  const TflOperator& op = d.ops[oi];
  FcGeometry g;
  const char* why = "";
  if (!FcArgs(d, op, &g, &why)) return Refused(op, why);
  const TflTensor& in = d.tensors[op.inputs[0]];
  const TflTensor& w = d.tensors[g.filter];
  const TflTensor& out = d.tensors[op.outputs[0]];
  const bool i8 = in.type == DataType::kInt8;
  const int32_t* bias = g.bias >= 0 ? reinterpret_cast<const int32_t*>(d.tensors[g.bias].data) : nullptr;
  const int units = g.units, depth = g.depth, rows = g.rows;
  const int depth_pad = (depth + 15) / 16 * 16;
  int32_t mult, shift, amin, amax;
  FullyConnectedMultiplier(Scale(in), Scale(w), Scale(out), &mult, &shift);
  ActivationRangeQuantized(g.act, Scale(out), Zp(out), i8, &amin, &amax);
  const int32_t in_zp = Dom(in), w_zp = Dom(w);
  const size_t wbytes = static_cast<size_t>(units) * depth_pad;
  std::shared_ptr<DeviceBlob> blob;
  RETURN_STATUS_IF(ConstBlob(ckey, wbytes + 12ull * units, sg, [&](uint8_t* host) {
    int8_t* packed = reinterpret_cast<int8_t*>(host);
    int32_t* tables = reinterpret_cast<int32_t*>(host + wbytes);
    for (int u = 0; u < units; ++u) {
      int64_t s = 0;
      for (int k = 0; k < depth; ++k) {
        const uint8_t raw = w.data[static_cast<size_t>(u) * depth + k];
        const int v = i8 ? static_cast<int>(static_cast<int8_t>(raw)) : static_cast<int>(raw) - 128;
        packed[static_cast<size_t>(u) * depth_pad + k] = static_cast<int8_t>(v);
        s += v;
      }
      tables[u] = static_cast<int32_t>((bias ? bias[u] : 0) - static_cast<int64_t>(in_zp) * s +
                                       static_cast<int64_t>(depth) * in_zp * w_zp);
      tables[units + u] = mult;
      tables[2 * units + u] = shift;
    }
    return absl::OkStatus();
  }, &blob));
  const int32_t* tab = reinterpret_cast<const int32_t*>(static_cast<char*>(blob->ptr()) + wbytes);
  bh_fc_params& p = L->Set<Launch::kFc>();
  p.rows = rows; p.depth = depth; p.depth_pad = depth_pad; p.units = units;
  p.in_xor = i8 ? 0 : 0x80; p.in_zp = in_zp; p.w_zp = w_zp; p.out_zp = Zp(out);
  p.act_min = amin; p.act_max = amax; p.input = in_ptr; p.output = out_ptr;
  p.weights = static_cast<const int8_t*>(blob->ptr());
  p.bias_eff = tab; p.mult = tab + units; p.shift = tab + 2 * units;
  L->kernel = "fc_kernel";
  L->alg_ops = 2.0 * rows * units * depth;
  L->alg_bytes = static_cast<double>(rows) * depth + static_cast<double>(rows) * units +
                 static_cast<double>(units) * depth + 12.0 * units;
  return absl::OkStatus();
}

// Hybrid FULLY_CONNECTED (float32 input, int8 filter).  Two launches: the
// input's rows quantised into a scratch owned by this subgraph (q, then one
// scale and one offset per row), then the int8 product with the float
// epilogue.  The constant blob holds the filter packed as the int8 FC packs
// it (K padded to 16 by zeros), the row sums sum_k w[u][k] and the bias.
absl::Status HipModelExecutor::LowerFcHybrid(const HipModel& model, int oi, void* in_ptr, void* out_ptr,
                                             const std::string& ckey, PreparedSubgraph* sg, Launch* L) {
  const TflModel& d = model.desc();
  const TflOperator& op = d.ops[oi];
  HybridFcGeometry h;
  const char* why = "";
  if (!HybridFcArgs(d, op, &h, &why)) return Refused(op, why);
  const FcGeometry& g = h.fc;
  const TflTensor& w = d.tensors[g.filter];
  const int units = g.units, depth = g.depth, rows = g.rows;
  const int depth_pad = (depth + 15) / 16 * 16;
  const size_t wbytes = static_cast<size_t>(units) * depth_pad;
  const std::vector<float> bias = g.bias >= 0 ? FloatData(d, g.bias) : std::vector<float>();
  std::shared_ptr<DeviceBlob> blob;
  RETURN_STATUS_IF(ConstBlob(ckey + "/hybrid", wbytes + 8ull * units, sg, [&](uint8_t* host) {
    int8_t* packed = reinterpret_cast<int8_t*>(host);
    int32_t* sums = reinterpret_cast<int32_t*>(host + wbytes);
    float* b = reinterpret_cast<float*>(host + wbytes + 4ull * units);
    for (int u = 0; u < units; ++u) {
      int32_t s = 0;
      for (int k = 0; k < depth; ++k) {
        const int8_t v = static_cast<int8_t>(w.data[static_cast<size_t>(u) * depth + k]);
        packed[static_cast<size_t>(u) * depth_pad + k] = v;
        s += v;
      }
      sums[u] = s;
      b[u] = bias.empty() ? 0.f : bias[u];
    }
    return absl::OkStatus();
  }, &blob));
  // scratch: q [rows][depth] (padded to 16 bytes), scale [rows], offset [rows]
  const size_t qbytes = (static_cast<size_t>(rows) * depth + 15) / 16 * 16;
  auto scratch = std::make_shared<DeviceBlob>(ordinal_, qbytes + 8ull * rows);
  if (!scratch->ok()) return absl::InternalError("HBM scratch allocation failed");
  sg->consts.push_back(scratch);
  char* sp = static_cast<char*>(scratch->ptr());
  const bool cpu = device_flag_ == DeviceFlag::kCPU;
  Launch Q;
  Q.op_index = oi;
  bh_dynquant_params dq{};
  dq.rows = rows; dq.depth = depth; dq.asymmetric = h.asymmetric ? 1 : 0;
  dq.input = static_cast<const float*>(in_ptr);
  dq.q = reinterpret_cast<int8_t*>(sp);
  dq.scale = reinterpret_cast<float*>(sp + qbytes);
  dq.offset = reinterpret_cast<int32_t*>(sp + qbytes + 4ull * rows);
  Q.Set<Launch::kDynQuantRows>(dq);
  Q.kernel = cpu ? "dynquant_rows_host" : bh_dynquant_rows_kernel(&dq);
  Q.alg_bytes = 5.0 * rows * depth + 8.0 * rows;
  sg->launches.push_back(Q);
  const char* base = static_cast<const char*>(blob->ptr());
  bh_fc_hybrid_params& p = L->Set<Launch::kFcHybrid>();
  p.rows = rows; p.depth = depth; p.depth_pad = depth_pad; p.units = units;
  p.w_scale = h.w_scale;
  FloatActRange(g.act, &p.act_min, &p.act_max);
  p.q = dq.q; p.in_scale = dq.scale; p.in_offset = dq.offset;
  p.weights = reinterpret_cast<const int8_t*>(base);
  p.w_row_sum = reinterpret_cast<const int32_t*>(base + wbytes);
  p.bias = g.bias >= 0 ? reinterpret_cast<const float*>(base + wbytes + 4ull * units) : nullptr;
  p.output = static_cast<float*>(out_ptr);
  L->kernel = cpu ? "fc_hybrid_host" : bh_fc_hybrid_kernel(&p);
  L->alg_ops = 2.0 * rows * units * depth;
  L->alg_bytes = static_cast<double>(rows) * depth + 8.0 * rows + 4.0 * rows * units +
                 static_cast<double>(units) * depth + 8.0 * units;
  return absl::OkStatus();
}

// Hybrid CONV_2D / DEPTHWISE_CONV_2D (float32 input, int8 filter; executors
// built with BAND_HIP_HYBRID_CONV=1).  The input's batch items are quantised
// into a scratch owned by this subgraph (q, the chunk pairs of the two-launch
// form, then one scale and one offset per item; a job-batch variant has more
// items and so a larger scratch), then the int8 product with the float
// epilogue.  One constant blob per op, shared across executors: the filter
// (CONV_2D: packed [out_c][k_pad], K padded to 16 by zeros; depthwise: as the
// flatbuffer holds it), the row sums over all taps, the scales expanded to
// [out_c] and the bias.
absl::Status HipModelExecutor::LowerConvHybrid(const HipModel& model, int oi, void* in_ptr, void* out_ptr,
                                               const std::string& ckey, PreparedSubgraph* sg, Launch* L) {
  const TflModel& d = model.desc();
  const TflOperator& op = d.ops[oi];
  HybridConvGeometry h;
  const char* why = "";
  if (!HybridConvArgs(d, op, &h, &why)) return Refused(op, why);
  const ConvGeometry& g = h.conv;
  const TflTensor& w = d.tensors[g.filter];
  const bool dw = h.depthwise;
  const int oc = g.out_c;
  const int K = g.k_h * g.k_w * (dw ? 1 : g.in_c);
  const int k_pad = (K + 15) / 16 * 16;
  const size_t wbytes = dw ? (static_cast<size_t>(K) * oc + 15) / 16 * 16 : static_cast<size_t>(oc) * k_pad;
  const std::vector<float> bias = g.bias >= 0 ? FloatData(d, g.bias) : std::vector<float>();
  std::shared_ptr<DeviceBlob> blob;
  RETURN_STATUS_IF(ConstBlob(ckey + "/hybrid", wbytes + 12ull * oc, sg, [&](uint8_t* host) {
    int8_t* packed = reinterpret_cast<int8_t*>(host);
    int32_t* sums = reinterpret_cast<int32_t*>(host + wbytes);
    float* scales = reinterpret_cast<float*>(host + wbytes + 4ull * oc);
    float* b = reinterpret_cast<float*>(host + wbytes + 8ull * oc);
    std::memset(host, 0, wbytes);
    for (int c = 0; c < oc; ++c) {
      int32_t s = 0;
      for (int k = 0; k < K; ++k) {
        // OHWI: [c][k]; depthwise [1][kh][kw][oc]: [k][c]
        const size_t at = dw ? static_cast<size_t>(k) * oc + c : static_cast<size_t>(c) * K + k;
        const int8_t v = static_cast<int8_t>(w.data[at]);
        packed[dw ? at : static_cast<size_t>(c) * k_pad + k] = v;
        s += v;
      }
      sums[c] = s;
      scales[c] = h.w_scale[c];
      b[c] = bias.empty() ? 0.f : bias[c];
    }
    return absl::OkStatus();
  }, &blob));
  // scratch: q (padded to 16 bytes), pairs [items][chunks][2], scale [items], offset [items]
  const int items = g.batch;
  const int item_size = g.in_h * g.in_w * g.in_c;
  const size_t chunks = (static_cast<size_t>(item_size) + BH_DYNQUANT_CHUNK - 1) / BH_DYNQUANT_CHUNK;
  const size_t qbytes = (static_cast<size_t>(items) * item_size + 15) / 16 * 16;
  const size_t pbytes = 8ull * items * chunks;
  auto scratch = std::make_shared<DeviceBlob>(ordinal_, qbytes + pbytes + 8ull * items);
  if (!scratch->ok()) return absl::InternalError("HBM scratch allocation failed");
  sg->consts.push_back(scratch);
  char* sp = static_cast<char*>(scratch->ptr());
  const bool cpu = device_flag_ == DeviceFlag::kCPU;
  Launch Q;
  Q.op_index = oi;
  bh_dynquant_items_params dqi{};
  dqi.items = items; dqi.item_size = item_size; dqi.asymmetric = h.per_channel ? 1 : 0;
  dqi.input = static_cast<const float*>(in_ptr);
  dqi.q = reinterpret_cast<int8_t*>(sp);
  dqi.pairs = reinterpret_cast<float*>(sp + qbytes);
  dqi.scale = reinterpret_cast<float*>(sp + qbytes + pbytes);
  dqi.offset = reinterpret_cast<int32_t*>(sp + qbytes + pbytes + 4ull * items);
  Q.Set<Launch::kDynQuantItems>(dqi);
  Q.kernel = cpu ? "dynquant_items_host" : bh_dynquant_items_kernel(&dqi);
  Q.alg_bytes = 5.0 * items * item_size + 8.0 * items;
  sg->launches.push_back(Q);
  const char* base = static_cast<const char*>(blob->ptr());
  bh_conv_hybrid_params& p = L->Set(dw ? Launch::kDwConvHybrid : Launch::kConvHybrid, bh_conv_hybrid_params{});
  p.batch = g.batch; p.in_h = g.in_h; p.in_w = g.in_w; p.in_c = g.in_c;
  p.out_h = g.out_h; p.out_w = g.out_w; p.out_c = oc;
  p.k_h = g.k_h; p.k_w = g.k_w; p.stride_h = g.stride_h; p.stride_w = g.stride_w;
  p.dil_h = g.dil_h; p.dil_w = g.dil_w; p.pad_h = g.pad_h; p.pad_w = g.pad_w;
  p.k_pad = k_pad;
  p.depth_multiplier = g.depth_multiplier;
  p.per_channel = h.per_channel ? 1 : 0;
  FloatActRange(g.act, &p.act_min, &p.act_max);
  p.q = dqi.q; p.in_scale = dqi.scale; p.in_offset = dqi.offset;
  p.weights = reinterpret_cast<const int8_t*>(base);
  p.w_row_sum = reinterpret_cast<const int32_t*>(base + wbytes);
  p.w_scale = reinterpret_cast<const float*>(base + wbytes + 4ull * oc);
  p.bias = g.bias >= 0 ? reinterpret_cast<const float*>(base + wbytes + 8ull * oc) : nullptr;
  p.output = static_cast<float*>(out_ptr);
  L->kernel = cpu ? (dw ? "dwconv_hybrid_host" : "conv_hybrid_host")
                  : (dw ? bh_dwconv2d_hybrid_kernel(&p) : bh_conv2d_hybrid_kernel(&p));
  const double outs = static_cast<double>(g.batch) * g.out_h * g.out_w * oc;
  L->alg_ops = 2.0 * outs * K;
  L->alg_bytes = static_cast<double>(items) * item_size + 8.0 * items + 4.0 * outs + static_cast<double>(wbytes) + 12.0 * oc;
  return absl::OkStatus();
}

// ADD / SUB / MUL int8 / uint8, SQUARED_DIFFERENCE int8
absl::Status HipModelExecutor::LowerEltwise(const HipModel& model, int oi, void* in_ptr, void* out_ptr,
                                            PreparedSubgraph* sg, Launch* L) {
  const TflModel& d = model.desc();
  const TflOperator& op = d.ops[oi];
  BroadcastShapes s;
  const char* why = "";
  if (!BroadcastArgs(d, op, &s, &why)) return Refused(op, why);
  const TflTensor& in = d.tensors[op.inputs[0]];
  const TflTensor& b = d.tensors[op.inputs[1]];
  const TflTensor& out = d.tensors[op.outputs[0]];
  const bool i8 = in.type == DataType::kInt8;
  void* b_ptr = nullptr;
  RETURN_STATUS_IF(DevicePtr(model, op.inputs[1], sg, &b_ptr));
  bh_eltwise_params& p = L->Set<Launch::kEltwise>();
  p.in_signed = i8 ? 1 : 0;
  std::copy_n(s.a, 4, p.shape_a); std::copy_n(s.b, 4, p.shape_b); std::copy_n(s.o, 4, p.shape_o);
  p.a_off = -Zp(in); p.b_off = -Zp(b); p.o_off = Zp(out);
  ActivationRangeQuantized(op.options.Int8(0, 0), Scale(out), Zp(out), i8, &p.act_min, &p.act_max);
  if (op.builtin == kTflSquaredDifference) {
    AddParams ap;
    if (!SquaredDifferenceArgs(d, op, nullptr, &ap, &why)) return Refused(op, why);
    p.kind = BH_ELT_SQDIFF;
    p.left_shift = ap.left_shift;
    p.a_mult = ap.m1; p.a_shift = ap.s1;
    p.b_mult = ap.m2; p.b_shift = ap.s2;
    p.o_mult = ap.mo; p.o_shift = ap.so;
    p.act_min = -128; p.act_max = 127;  // SquaredDifferenceOptions has no fused activation
  } else if (op.builtin == kTflMul) {
    p.kind = BH_ELT_MUL;
    MulMultiplier(Scale(in), Scale(b), Scale(out), &p.o_mult, &p.o_shift);
  } else {
    p.kind = BH_ELT_ADD;
    const AddParams ap = AddSubParams(Scale(in), Scale(b), Scale(out), op.builtin == kTflSub);
    p.left_shift = ap.left_shift;
    p.a_mult = ap.m1; p.a_shift = ap.s1;
    p.b_mult = ap.m2; p.b_shift = ap.s2;
    p.o_mult = ap.mo; p.o_shift = ap.so;
  }
  p.a = in_ptr; p.b = b_ptr; p.out = out_ptr;
  L->kernel = p.kind != BH_ELT_SQDIFF                 ? "eltwise_kernel"
              : device_flag_ == DeviceFlag::kCPU ? "eltwise_sqdiff_host"
                                                 : "eltwise_sqdiff_kernel";
  L->alg_bytes = static_cast<double>(in.num_elements() + b.num_elements() + out.num_elements());
  return absl::OkStatus();
}

// AVERAGE_POOL_2D / MAX_POOL_2D int8 / uint8
absl::Status HipModelExecutor::LowerPool(const HipModel& model, int oi, void* in_ptr, void* out_ptr, Launch* L) {
  const TflModel& d = model.desc();
  const TflOperator& op = d.ops[oi];
  PoolGeometry g;
  const char* why = "";
  if (!PoolArgs(d, op, &g, &why)) return Refused(op, why);
  const TflTensor& in = d.tensors[op.inputs[0]];
  const TflTensor& out = d.tensors[op.outputs[0]];
  const bool i8 = in.type == DataType::kInt8;
  bh_pool_params& p = L->Set<Launch::kPool>();
  p.kind = op.builtin == kTflAveragePool2D ? BH_POOL_AVG : BH_POOL_MAX;
  p.in_signed = i8 ? 1 : 0;
  SetGeometry(g, &p);
  ActivationRangeQuantized(g.act, Scale(out), Zp(out), i8, &p.act_min, &p.act_max);
  p.input = in_ptr; p.output = out_ptr;
  L->kernel = "pool_kernel";
  L->alg_bytes = static_cast<double>(in.num_elements() + out.num_elements());
  return absl::OkStatus();
}

// MEAN: host kernel on a CPU worker, mean_kernel on the GPU
absl::Status HipModelExecutor::LowerMean(const HipModel& model, int oi, void* in_ptr, void* out_ptr, Launch* L) {
  const TflModel& d = model.desc();
  const TflOperator& op = d.ops[oi];
  const TflTensor& in = d.tensors[op.inputs[0]];
  const TflTensor& out = d.tensors[op.outputs[0]];
  MeanGeometry g;
  const char* why = "";
  if (!MeanArgs(d, op, &g, &why)) return Refused(op, why);
  L->alg_bytes = static_cast<double>(meta_[op.inputs[0]]->bytes + meta_[op.outputs[0]]->bytes);
  if (g.rows) {
    // the last axis of an 8-bit tensor: one wave per row (mean_rows_kernel / CpuMeanRows)
    bh_mean_rows_params& q = L->Set<Launch::kMeanRows>();
    q.rows = g.outer;
    q.depth = static_cast<int>(g.reduce);
    q.type = in.type == DataType::kInt8 ? 1 : 2;
    q.exact = g.exact ? 1 : 0;
    // reference_ops::QuantizedMeanOrSum: float32, each operation on its own
    q.scale = Scale(in) / Scale(out);
    q.bias = -static_cast<float>(Zp(in)) * q.scale + 0.5f;
    q.out_zp = Zp(out);
    q.input = in_ptr; q.output = out_ptr;
    if (bh_mean_rows_check(&q) != 0) return absl::InternalError(std::string("MEAN: ") + bh_last_error());
    L->kernel = device_flag_ == DeviceFlag::kGPU ? bh_mean_rows_kernel(&q) : "mean_rows_host";
    return absl::OkStatus();
  }
  bh_mean_params& p = L->Set<Launch::kMean>();
  p.outer = g.outer; p.reduce = g.reduce; p.inner = g.inner;
  p.type = in.type == DataType::kFloat32 ? 0 : (in.type == DataType::kInt8 ? 1 : 2);
  if (p.type) {
    // optimized_integer_ops::Mean (TFLite 2.9.2): the float products as
    // written there, then QuantizeMultiplier of the float scale
    const float in_scale = Scale(in), out_scale = Scale(out);
    const float n = static_cast<float>(p.reduce);
    p.bias = Zp(out) - static_cast<int32_t>(Zp(in) * in_scale / out_scale);
    const float real_scale = in_scale / (n * out_scale);
    int shift = 0;
    QuantizeMultiplier(static_cast<double>(real_scale), &p.multiplier, &shift);
    p.shift = shift;
  }
  p.input = in_ptr; p.output = out_ptr;
  L->kernel = device_flag_ == DeviceFlag::kGPU ? "mean_kernel" : "mean_host";
  L->alg_bytes = static_cast<double>(meta_[op.inputs[0]]->bytes + meta_[op.outputs[0]]->bytes);
  return absl::OkStatus();
}

absl::Status HipModelExecutor::LowerArgMinMax(const HipModel& model, int oi, void* in_ptr, void* out_ptr, Launch* L) {
  const TflModel& d = model.desc();
  const TflOperator& op = d.ops[oi];
  const DataType type = d.tensors[op.inputs[0]].type;
  bh_argminmax_params& p = L->Set<Launch::kArgMinMax>();
  if (!ArgMinMaxArgs(d, op, &p.outer, &p.axis_len, &p.inner, &p.out_bytes))
    return absl::InternalError("unsupported ARG_MAX / ARG_MIN");
  p.in_type = type == DataType::kFloat32 ? BH_ARG_F32 : (type == DataType::kInt8 ? BH_ARG_I8 : BH_ARG_U8);
  p.is_min = op.builtin == kTflArgMin ? 1 : 0;
  p.input = in_ptr; p.output = out_ptr;
  L->kernel = device_flag_ == DeviceFlag::kCPU ? "argminmax_host" : bh_argminmax_kernel(&p);
  L->alg_bytes = static_cast<double>(meta_[op.inputs[0]]->bytes + meta_[op.outputs[0]]->bytes);
  return absl::OkStatus();
}

// TFLite_Detection_PostProcess on the CPU worker (CpuSupports)
absl::Status HipModelExecutor::LowerDetectionHost(const HipModel& model, int oi, void* in_ptr, PreparedSubgraph* sg,
                                                  Launch* L) {
  const TflModel& d = model.desc();
  const TflOperator& op = d.ops[oi];
  CpuDetectionParams& p = L->Set<Launch::kDetectionPost>();
  if (!DetectionSupported(d, op, &p)) return absl::InternalError("unsupported custom op " + op.custom_code);
  void* scores = nullptr;
  void* anchors = nullptr;
  void* outs[4];
  RETURN_STATUS_IF(DevicePtr(model, op.inputs[1], sg, &scores));
  RETURN_STATUS_IF(DevicePtr(model, op.inputs[2], sg, &anchors));
  for (int k = 0; k < 4; ++k) RETURN_STATUS_IF(DevicePtr(model, op.outputs[k], sg, &outs[k]));
  p.box_encodings = static_cast<const float*>(in_ptr);
  p.class_scores = static_cast<const float*>(scores);
  p.anchors = static_cast<const float*>(anchors);
  p.out_boxes = static_cast<float*>(outs[0]);
  p.out_classes = static_cast<float*>(outs[1]);
  p.out_scores = static_cast<float*>(outs[2]);
  p.out_num = static_cast<float*>(outs[3]);
  L->kernel = "detection_postprocess_host";
  return absl::OkStatus();
}

absl::Status HipModelExecutor::Lower(const HipModel& model, int oi, PreparedSubgraph* sg) {
  const TflModel& d = model.desc();
  const TflOperator& op = d.ops[oi];
  std::string why;
  const bool cpu = device_flag_ == DeviceFlag::kCPU;
  if (!(cpu ? CpuSupportsHere(d, op, &why) : GpuSupportsHere(d, op, &why)))
    return absl::InternalError("HIP backend cannot run op " + std::to_string(oi) + " (" +
                               TflBuiltinName(op.builtin) + ") on " + ToString(device_flag_) + ": " + why);
  if (DequantFoldsIntoDetection(d, *sg, oi)) {
    // the detection kernels read the 8-bit tensor: no launch, no float tensor
    sg->fused_tensors.insert(op.outputs[0]);
    return absl::OkStatus();
  }
  if (IsReindexOp(op.builtin)) return LowerReindex(model, oi, sg);
  if (op.builtin == kTflGather || op.builtin == kTflEmbeddingLookup) return LowerGather(model, oi, sg);
  void* in_ptr = nullptr;
  void* out_ptr = nullptr;
  RETURN_STATUS_IF(DevicePtr(model, op.inputs[0], sg, &in_ptr));
  RETURN_STATUS_IF(DevicePtr(model, op.outputs[0], sg, &out_ptr));
  const std::string ckey = "m" + Hex(model.serial()) + "/op" + std::to_string(oi);
  Launch L;
  L.op_index = oi;
  L.out_tensor = op.outputs[0];
  bool emit = true;
  auto lower = [&]() -> absl::Status {
    switch (op.builtin) {
      case kTflConv2D: return LowerConv(model, oi, in_ptr, out_ptr, ckey, sg, &L);
      case kTflDepthwiseConv2D: return LowerDepthwise(model, oi, in_ptr, out_ptr, ckey, sg, &L);
      case kTflFullyConnected: return LowerFc(model, oi, in_ptr, out_ptr, ckey, sg, &L);
      case kTflTransposeConv: return LowerTransposeConv(model, oi, out_ptr, ckey, sg, &L);
      case kTflAdd: case kTflSub: case kTflMul: case kTflSquaredDifference: return LowerEltwise(model, oi, in_ptr, out_ptr, sg, &L);
      case kTflAveragePool2D: case kTflMaxPool2D: return LowerPool(model, oi, in_ptr, out_ptr, &L);
      case kTflMean: return LowerMean(model, oi, in_ptr, out_ptr, &L);
      case kTflArgMax: case kTflArgMin: return LowerArgMinMax(model, oi, in_ptr, out_ptr, &L);
      case kTflBatchMatMul: return LowerBatchMatMul(model, oi, in_ptr, out_ptr, sg, &L);
      case kTflCustom:
        return cpu ? LowerDetectionHost(model, oi, in_ptr, sg, &L) : LowerDetectionGpu(model, oi, sg, &L);
      case kTflCast: {  // equal types: a copy; else a converting copy (cast_kernel / CpuCast)
        int from = 0, to = 0;
        const char* why = "";
        if (!CastArgs(d, op, &from, &to, &why)) return Refused(op, why);
        const size_t bytes = meta_[op.outputs[0]]->bytes;
        CopyArgs c{out_ptr, in_ptr, bytes};
        if (from != to) {
          c.cast_from = from;
          c.cast_to = to;
          c.count = static_cast<long>(d.tensors[op.outputs[0]].num_elements());
        }
        L.Set<Launch::kCopy>(c);
        L.kernel = from == to ? "copy" : (cpu ? "cast_host" : "cast_kernel");
        L.alg_bytes = static_cast<double>(meta_[op.inputs[0]]->bytes + bytes);
        emit = from != to || in_ptr != out_ptr;
        return absl::OkStatus();
      }
      case kTflReshape: case kTflSqueeze:  // same bytes, new dims
        L.Set<Launch::kCopy>({out_ptr, in_ptr, meta_[op.outputs[0]]->bytes});
        L.kernel = "copy";
        L.alg_bytes = 2.0 * meta_[op.outputs[0]]->bytes;
        emit = in_ptr != out_ptr;  // aliased slot: nothing to move
        return absl::OkStatus();
      default: return LowerGlue(model, oi, in_ptr, out_ptr, ckey, sg, &L);
    }
  };
  RETURN_STATUS_IF(IsFloatOp(d, op) ? LowerFloat(model, oi, in_ptr, out_ptr, ckey, sg, &L, &emit) : lower());
  if (emit && L.kind() == Launch::kNone) return absl::InternalError("op " + std::to_string(oi) + " lowered to no launch");
  if (emit) sg->launches.push_back(L);
  return absl::OkStatus();
}

}  // namespace hip
}  // namespace band
