// Candidate order of TFLite_Detection_PostProcess's fast NMS as one
// comparable key (host and device): the reference sorts the candidates by
// score descending with a stable sort, i.e. ties by anchor index ascending.
//
//   key = monotone(score) << 32 | ~index
//
// so the larger key is drawn first.  monotone() maps a float to a uint32
// whose unsigned order is the float order; -0.0f and +0.0f compare equal in
// the reference and are canonicalised to one value.  No non-NaN score maps
// to 0 in the high word (-inf -> 0x007fffff), so key 0 is free as the "no
// candidate" value.  NaN scores are never candidates and must not be keyed.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define BH_DET_HD __host__ __device__
#else
#define BH_DET_HD
#endif

BH_DET_HD inline uint32_t bh_det_score_bits(float score) {
  if (score == 0.0f) score = 0.0f;  // -0.0f -> +0.0f
  uint32_t b;
  __builtin_memcpy(&b, &score, 4);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

BH_DET_HD inline float bh_det_bits_score(uint32_t m) {
  const uint32_t b = (m & 0x80000000u) ? (m & 0x7fffffffu) : ~m;
  float f;
  __builtin_memcpy(&f, &b, 4);
  return f;
}

BH_DET_HD inline uint64_t bh_det_key(float score, uint32_t index) {
  return (static_cast<uint64_t>(bh_det_score_bits(score)) << 32) | static_cast<uint32_t>(~index);
}

BH_DET_HD inline uint32_t bh_det_key_index(uint64_t key) { return ~static_cast<uint32_t>(key); }
BH_DET_HD inline float bh_det_key_score(uint64_t key) { return bh_det_bits_score(static_cast<uint32_t>(key >> 32)); }
