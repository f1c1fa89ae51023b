// Every environment variable the HIP backend reads: one typed reader per
// variable, called where the value is needed (nothing is cached here; a
// caller that wants a per-process value keeps it in a static of its own).
// INTEGRATION.md, "Environment", documents each one.
#ifndef BAND_BACKEND_HIP_ENV_H_
#define BAND_BACKEND_HIP_ENV_H_

#include <algorithm>
#include <climits>
#include <cstdlib>

namespace band {
namespace hip {
namespace env {

// unset: def.  A default-on flag is off only for a value starting with '0';
// a default-off flag is on only for one starting with '1'.
inline bool Flag(const char* name, bool def) {
  const char* v = std::getenv(name);
  return v ? (def ? v[0] != '0' : v[0] == '1') : def;
}
// unset: def; else the value, at least lo
inline int Int(const char* name, int def, int lo) {
  const char* v = std::getenv(name);
  return v ? std::max(lo, std::atoi(v)) : def;
}
// unset: ""
inline const char* Str(const char* name) {
  const char* v = std::getenv(name);
  return v ? v : "";
}

// 0: launches enqueued one by one instead of a captured graph's replay
inline bool Graph() { return Flag("BAND_HIP_GRAPH", true); }
// how a pass is waited for: block | poll | poller | spin | anything else: adaptive
inline const char* Sync() { return Str("BAND_HIP_SYNC"); }
// 0: job-batch I/O staged through the slot views instead of the caller's tensors
inline bool DirectIo() { return Flag("BAND_HIP_DIRECT_IO", true); }
// max jobs per coalesced pass (0 or 1: off)
inline int Coalesce() { return Int("BAND_HIP_COALESCE", 16, INT_MIN); }
// coalescer lanes per model and GPU
inline int CoalesceLanes() { return Int("BAND_HIP_COALESCE_LANES", 2, 1); }
// how long a free lane waits for more jobs, in microseconds
inline int CoalesceWaitUs() { return Int("BAND_HIP_COALESCE_WAIT_US", 100, 0); }
// dma: lanes copy the members' tensors themselves; anything else: copy
inline const char* CoalesceIo() { return Str("BAND_HIP_COALESCE_IO"); }
// test hook: the lane build fails as it would out of device memory
inline bool CoalesceFailBuild() { return Int("BAND_HIP_COALESCE_FAIL_BUILD", 0, INT_MIN) != 0; }
// 1: TFLite_Detection_PostProcess on the device
inline bool GpuDetection() { return Flag("BAND_HIP_GPU_DETECTION", false); }
// 1: hybrid CONV_2D / DEPTHWISE_CONV_2D (float32 input, int8 filter) run, on both workers
inline bool HybridConv() { return Flag("BAND_HIP_HYBRID_CONV", false); }
// 0: job-batch variants capture their graphs lazily
inline bool Precapture() { return Flag("BAND_HIP_PRECAPTURE", true); }
// 1: BATCH_MATMUL -> SOFTMAX -> BATCH_MATMUL (int8) as one attention_i8_kernel launch on kGPU executors
inline bool FusedAttention() { return Flag("BAND_HIP_FUSED_ATTENTION", false); }
// 1: the ten float32 ops of a LayerNorm as one layernorm_f32_kernel launch on kGPU executors, which also
// quantises its rows for the hybrid FULLY_CONNECTEDs that read them
inline bool FusedLayerNormF32() { return Flag("BAND_HIP_FUSED_LAYERNORM_F32", false); }
// 1: kernels without the host copies (tools/concurrency_probe.py --no-io)
inline bool ProbeNoIo() { return Flag("BAND_HIP_PROBE_NO_IO", false); }
// file the chain tuner's decisions persist in (unset or empty: none)
inline const char* TuneFile() { return Str("BAND_HIP_TUNE_FILE"); }
// 0: fused forms picked by the static model, nothing measured
inline bool Autotune() { return Flag("BAND_HIP_AUTOTUNE", true); }
// 0 | noirb | noadd | nochain | nogroup | noargmax | notile | nodeep | nosplit |
// nostage | nolayernorm | forcechain | forcetile | forcedeep | forcestage | forcedense
inline const char* Fusion() { return Str("BAND_HIP_FUSION"); }
// 0: threads that drive a GPU stay off its NUMA node's CPUs
inline bool NumaPin() { return Flag("BANDX_NUMA_PIN", true); }

}  // namespace env
}  // namespace hip
}  // namespace band

#endif  // BAND_BACKEND_HIP_ENV_H_
