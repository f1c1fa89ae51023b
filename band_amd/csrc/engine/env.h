// Every environment variable the engine reads: one typed reader per
// variable, called where the value is needed (nothing is cached here).
// INTEGRATION.md, "Environment", documents each one.
#ifndef BAND_ENGINE_ENV_H_
#define BAND_ENGINE_ENV_H_

#include <algorithm>
#include <cstdlib>

namespace band {
namespace env {

// unset: def; else the value, at least lo
inline long Int(const char* name, long def, long lo) {
  const char* v = std::getenv(name);
  return v ? std::max(lo, std::atol(v)) : def;
}

// request driver: threads that copy requests into the rings
inline int DriverLanes() { return static_cast<int>(Int("BANDX_DRIVER_LANES", 1, 1)); }
// request driver: requests of one model per RequestAsync call (def: the caller's hint)
inline int DriverBurst(int def) { return static_cast<int>(Int("BANDX_DRIVER_BURST", def, 1)); }
// request driver: threads that copy results out
inline int DriverReaders() { return static_cast<int>(Int("BANDX_DRIVER_READERS", 6, 1)); }
// request slots per model (the reference's 128)
inline int RequestRingSlots() { return static_cast<int>(Int("BANDX_REQUEST_RING_SLOTS", 128, 1)); }
// how long AcquireForWrite waits for a held output slot, in milliseconds
inline long OutputHoldMs() { return Int("BANDX_OUTPUT_HOLD_MS", 2000, 0); }

}  // namespace env
}  // namespace band

#endif  // BAND_ENGINE_ENV_H_
