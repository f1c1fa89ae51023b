// Stand-alone driver of the Args functions (backend/hip/lower_args.h): parses
// the .tflite files named on the command line and calls the Args function of
// every op's family, printing "ok" or the reason.  Built with
// -fsanitize=address,undefined by tests/test_lower_args_native.py; links only
// tflite_reader.cc, lower_args.cc, quant.cc and compat/band/common.cc.
#include <cstdio>
#include <string>
#include <vector>

#include "backend/hip/lower_args.h"

using namespace band::hip;

static const char* Check(const TflModel& m, const TflOperator& op) {
  const char* why = "refused";
  bool ok = true;
  switch (op.builtin) {
    case kTflConv2D:
    case kTflDepthwiseConv2D:
    case kTflTransposeConv: {
      ex::ConvGeometry g;
      ok = ex::ConvArgs(m, op, &g, &why);
      break;
    }
    case kTflFullyConnected: {
      ex::FcGeometry g;
      ok = ex::FcArgs(m, op, &g, &why);
      break;
    }
    case kTflAveragePool2D:
    case kTflMaxPool2D: {
      ex::PoolGeometry g;
      ok = ex::PoolArgs(m, op, &g, &why);
      break;
    }
    case kTflAdd:
    case kTflSub:
    case kTflMul:
    case kTflSquaredDifference: {
      ex::BroadcastShapes s;
      ok = ex::BroadcastArgs(m, op, &s, &why);
      break;
    }
    case kTflBatchMatMul: {
      bh_batch_matmul_params p;
      ok = ex::BatchMatMulArgs(m, op, &p, &why);
      break;
    }
    case kTflMean: {
      long o, r, i;
      ok = ex::MeanArgs(m, op, &o, &r, &i);
      break;
    }
    case kTflArgMax:
    case kTflArgMin: {
      long o, l, i;
      int bytes;
      ok = ex::ArgMinMaxArgs(m, op, &o, &l, &i, &bytes, nullptr, &why);
      break;
    }
    case kTflMirrorPad: {
      std::vector<int64_t> pads;
      int mode = 0;
      ok = ex::MirrorPadArgs(m, op, &pads, &mode);
      break;
    }
    case kTflCustom:
      ok = ex::DetectionSupported(m, op, nullptr);
      break;
    default:
      if (!ex::IsReindexOp(op.builtin)) return "no Args function";
      for (int k = 0; ok && k < static_cast<int>(op.outputs.size()); ++k) {
        bh_reindex_params map;
        ok = ex::ReindexArgs(m, op, k, &map, &why);
      }
  }
  return ok ? "ok" : why;
}

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    std::vector<uint8_t> bytes;
    FILE* f = std::fopen(argv[a], "rb");
    if (!f) {
      std::printf("%s: cannot open\n", argv[a]);
      return 2;
    }
    uint8_t chunk[4096];
    for (size_t n; (n = std::fread(chunk, 1, sizeof(chunk), f)) > 0;) bytes.insert(bytes.end(), chunk, chunk + n);
    std::fclose(f);
    TflModel m;
    std::string err;
    if (!m.Parse(bytes.data(), bytes.size(), &err)) {
      std::printf("%s: %s\n", argv[a], err.c_str());
      return 2;
    }
    for (size_t i = 0; i < m.ops.size(); ++i)
      std::printf("%s op %zu %s: %s\n", argv[a], i, TflBuiltinName(m.ops[i].builtin), Check(m, m.ops[i]));
  }
  return 0;
}
