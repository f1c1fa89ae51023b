// Host-only unit test of the detection postprocess's candidate key
// (kernels/det_key.hpp): sorting by the key descending is the reference's
// std::stable_sort by score descending (ties by index ascending), -0.0f and
// +0.0f are one score, the key is injective in the index and never 0, and the
// score is recovered from the key.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <set>
#include <vector>

#include "kernels/det_key.hpp"

static int failures = 0;
#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      ++failures;                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);   \
    }                                                           \
  } while (0)

static float FromBits(uint32_t b) {
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}

static void CheckOrder(const std::vector<float>& scores) {
  const size_t n = scores.size();
  std::vector<uint32_t> ref(n), got(n);
  for (size_t i = 0; i < n; ++i) ref[i] = got[i] = static_cast<uint32_t>(i);
  std::stable_sort(ref.begin(), ref.end(), [&](uint32_t a, uint32_t b) { return scores[a] > scores[b]; });
  std::sort(got.begin(), got.end(),
            [&](uint32_t a, uint32_t b) { return bh_det_key(scores[a], a) > bh_det_key(scores[b], b); });
  CHECK(ref == got);
  std::set<uint64_t> keys;
  for (size_t i = 0; i < n; ++i) {
    const uint64_t k = bh_det_key(scores[i], static_cast<uint32_t>(i));
    CHECK(k != 0);
    CHECK(bh_det_key_index(k) == i);
    CHECK(bh_det_key_score(k) == scores[i]);  // (-0.0f comes back as +0.0f: equal)
    keys.insert(k);
  }
  CHECK(keys.size() == n);
}

int main() {
  const float inf = std::numeric_limits<float>::infinity();
  const float edges[] = {0.0f, -0.0f, FromBits(1), FromBits(0x80000001u), FromBits(0x007fffffu),
                         FromBits(0x807fffffu), std::numeric_limits<float>::min(), -std::numeric_limits<float>::min(),
                         inf, -inf, std::numeric_limits<float>::max(), std::numeric_limits<float>::lowest(),
                         1.0f, -1.0f, 0.5f, 0.5f, 0.5f, std::nextafter(0.5f, 1.0f), std::nextafter(0.5f, 0.0f)};
  // the two zeros are one score, and order strictly against their neighbours
  CHECK(bh_det_score_bits(0.0f) == bh_det_score_bits(-0.0f));
  CHECK(bh_det_score_bits(FromBits(1)) > bh_det_score_bits(0.0f));
  CHECK(bh_det_score_bits(FromBits(0x80000001u)) < bh_det_score_bits(-0.0f));
  CHECK(bh_det_score_bits(-inf) != 0);
  // strict monotonicity over a sweep of bit patterns (non-NaN)
  {
    std::mt19937 rng(1);
    for (int i = 0; i < 200000; ++i) {
      const float a = FromBits(rng()), b = FromBits(rng());
      if (a != a || b != b) continue;
      CHECK((a < b) == (bh_det_score_bits(a) < bh_det_score_bits(b)));
      CHECK((a == b) == (bh_det_score_bits(a) == bh_det_score_bits(b)));
    }
  }
  // edge values, each several times, in a shuffled order
  {
    std::vector<float> s;
    for (int r = 0; r < 3; ++r)
      for (float e : edges) s.push_back(e);
    std::mt19937 rng(2);
    std::shuffle(s.begin(), s.end(), rng);
    CheckOrder(s);
  }
  // a few thousand random pairs: coarse scores (many ties), full-range bit
  // patterns, and a mix with the edge values
  for (int seed = 0; seed < 4; ++seed) {
    std::mt19937 rng(10 + seed);
    std::vector<float> s(4096);
    for (float& v : s) {
      const uint32_t r = rng();
      if (seed == 0) {
        v = static_cast<float>(r % 17) / 16.0f;
      } else if (seed == 1) {
        do v = FromBits(rng());
        while (v != v);
      } else if (r % 8 == 0) {
        v = edges[rng() % (sizeof(edges) / sizeof(edges[0]))];
      } else {
        v = static_cast<float>(static_cast<int>(r % 2001) - 1000) / 250.0f;
      }
    }
    CheckOrder(s);
  }
  // the index: every value of the low word is distinct and larger for the smaller index
  for (uint32_t i : {0u, 1u, 63u, 64u, 37628u, 0x7fffffffu, 0xfffffffeu}) {
    CHECK(bh_det_key(0.25f, i) > bh_det_key(0.25f, i + 1));
    CHECK(bh_det_key_index(bh_det_key(0.25f, i)) == i);
  }
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
