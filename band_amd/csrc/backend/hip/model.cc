#include "backend/hip/model.h"

#include <cstdio>

#include "backend/hip/lower_args.h"

namespace band {
namespace hip {

namespace {
std::atomic<uint64_t> g_next_serial{1};
}

HipModel::HipModel(ModelId id) : interface::IModel(id) {}

BackendType HipModel::GetBackendType() const { return BackendType::kTfLite; }

absl::Status HipModel::Load(std::vector<uint8_t>&& bytes) {
  initialized_ = false;
  bytes_ = std::move(bytes);
  std::string err;
  desc_ = TflModel();
  if (!desc_.Parse(bytes_.data(), bytes_.size(), &err)) return absl::InternalError("Invalid TFLite model: " + err);
  serial_ = g_next_serial.fetch_add(1);
  initialized_ = true;
  return absl::OkStatus();
}

absl::Status HipModel::FromPath(const char* filename) {
  path_ = filename ? filename : "";
  FILE* f = filename ? std::fopen(filename, "rb") : nullptr;
  if (!f) return absl::InternalError("Cannot load from file.");
  std::vector<uint8_t> bytes;
  std::fseek(f, 0, SEEK_END);
  const long n = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  if (n > 0) {
    bytes.resize(static_cast<size_t>(n));
    if (std::fread(bytes.data(), 1, bytes.size(), f) != bytes.size()) bytes.clear();
  }
  std::fclose(f);
  if (bytes.empty()) return absl::InternalError("Cannot load from file.");
  absl::Status s = Load(std::move(bytes));
  return s.ok() ? s : absl::InternalError("Cannot load from file.");
}

absl::Status HipModel::FromBuffer(const char* buffer, size_t buffer_size) {
  if (!buffer || buffer_size == 0) return absl::InternalError("Cannot load from buffer.");
  std::vector<uint8_t> bytes(reinterpret_cast<const uint8_t*>(buffer),
                             reinterpret_cast<const uint8_t*>(buffer) + buffer_size);
  absl::Status s = Load(std::move(bytes));
  return s.ok() ? s : absl::InternalError("Cannot load from buffer.");
}

absl::Status HipModel::CloneWithJobBatch(int batch, std::unique_ptr<HipModel>* out, bool gpu_detection) const {
  if (!initialized_) return absl::InternalError("job batching: model not loaded");
  if (batch < 1) return absl::InternalError("job batching: batch must be >= 1");
  for (const TflOperator& op : desc_.ops) {
    if (op.builtin == kTflCustom && !(gpu_detection && ex::DetectionSupported(desc_, op, nullptr)))
      return absl::InternalError("job batching: CUSTOM op " + op.custom_code);
    if (op.builtin == kTflConcatenation && op.options.valid() && !op.outputs.empty()) {
      const int rank = static_cast<int>(desc_.tensors[op.outputs[0]].shape.size());
      int axis = op.options.Int(0, 0);
      if (axis < 0) axis += rank;
      if (axis == 0) return absl::InternalError("job batching: CONCATENATION on the batch axis");
    }
    if (op.builtin == kTflArgMax || op.builtin == kTflArgMin) {
      long outer, len, inner;
      int out_bytes, axis = -1;
      if (ex::ArgMinMaxArgs(desc_, op, &outer, &len, &inner, &out_bytes, &axis) && axis == 0)
        return absl::InternalError(std::string("job batching: ") + TflBuiltinName(op.builtin) + " on the batch axis");
    }
    if (op.builtin == kTflMean) {
      // an 8-bit MEAN over the last axis never reduces axis 0 of a tensor of
      // rank >= 2; a rank-1 one (or a float MEAN from axis 0 on) would
      ex::MeanGeometry g;
      if (ex::MeanArgs(desc_, op, &g) && g.reduces_axis0)
        return absl::InternalError("job batching: MEAN over the batch axis");
    }
    if (op.builtin == kTflBatchMatMul) {
      // axis 0 must be a matmul batch dim of the output and of every
      // activation operand; a constant operand has to broadcast along it
      bool batch_axis_ok = false;
      if (ex::BatchMatMulArgs(desc_, op, nullptr, nullptr, &batch_axis_ok) && !batch_axis_ok) {
        bool rank2 = false;
        for (int k = 0; k < 2; ++k) {
          const TflTensor& t = desc_.tensors[op.inputs[k]];
          rank2 = rank2 || (!t.is_const() && t.shape.size() == 2);
        }
        return absl::InternalError(rank2 ? "job batching: BATCH_MATMUL with a rank-2 activation operand"
                                         : "job batching: BATCH_MATMUL operand does not broadcast along the batch axis");
      }
    }
    if (op.builtin == kTflGather) {
      // the embedding (constant params, axis 0, runtime indices) or an
      // activation gathered along an inner axis by constant indices
      bool batch_ok = false;
      const char* why = "";
      if (ex::GatherArgs(desc_, op, nullptr, &why, &batch_ok) && !batch_ok)
        return absl::InternalError(std::string("job batching: GATHER with ") + why);
    }
    if (op.builtin == kTflEmbeddingLookup) {  // GATHER's rule: a constant table, runtime ids
      bool batch_ok = false;
      const char* why = "";
      if (ex::EmbeddingLookupArgs(desc_, op, nullptr, &why, &batch_ok) && !batch_ok)
        return absl::InternalError(std::string("job batching: EMBEDDING_LOOKUP with ") + why);
    }
    if (op.builtin == kTflPack) {
      int axis = -1;
      if (ex::PackArgs(desc_, op, nullptr, nullptr, &axis) && axis == 0)
        return absl::InternalError("job batching: PACK on the batch axis");
    }
    if (ex::IsReindexOp(op.builtin)) {
      // a map may touch axis 0 only as the full range: no TRANSPOSE with
      // perm[0] != 0, no SPLIT / SPLIT_V / UNPACK on axis 0, no slice of part
      // of it, no TILE that repeats it
      for (int k = 0; k < static_cast<int>(op.outputs.size()); ++k) {
        bh_reindex_params map;
        bool whole_batch = false;
        if (ex::ReindexArgs(desc_, op, k, &map, nullptr, &whole_batch) && !whole_batch)
          return absl::InternalError(std::string("job batching: ") + TflBuiltinName(op.builtin) +
                                     " does not keep the whole batch axis");
      }
    }
  }
  for (const TflTensor& t : desc_.tensors)
    if (!t.is_const() && (t.shape.empty() || t.shape[0] != 1))
      return absl::InternalError("job batching: tensor '" + t.name + "' has no unit batch dimension");
  auto m = std::make_unique<HipModel>(id_);
  m->path_ = path_;
  std::vector<uint8_t> bytes = bytes_;
  absl::Status loaded = m->Load(std::move(bytes));
  if (!loaded.ok()) return loaded;
  for (TflTensor& t : m->desc_.tensors)
    if (!t.is_const()) t.shape[0] = batch;
  m->serial_ = serial_;
  *out = std::move(m);
  return absl::OkStatus();
}

}  // namespace hip
}  // namespace band
