// Launch (backend/hip/launch.h) alone, under AddressSanitizer and UBSan: for
// every kind, a launch made with that kind's payload reports the kind and
// gives the payload back through the pointer accessor of its type and of no
// other type; a copy and a move hold the same payload; conv_if() / conv()
// answer for kConv and kConvGrouped alone.  The reference accessors' stop on a
// mismatch is not run.
#include <cstdint>
#include <cstdio>
#include <utility>

#include "backend/hip/launch.h"

using band::hip::ConvGroupArgs;
using band::hip::Launch;
using band::hip::LayerNormArgs;

namespace {

int g_failed = 0;
#define CHECK(cond, k)                                                              \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      std::printf("FAIL kind %d line %d: %s\n", static_cast<int>(k), __LINE__, #cond); \
      ++g_failed;                                                                   \
    }                                                                               \
  } while (0)

// One pointer field of every parameter block, the first of these it has:
// the mark a payload carries through the launch
template <int N>
struct Rank : Rank<N - 1> {};
template <>
struct Rank<0> {};
#define SLOT(rank, field)                                   \
  template <class P>                                        \
  auto Slot(P& p, Rank<rank>) -> decltype((p.field)) {      \
    return p.field;                                         \
  }
SLOT(8, output)
SLOT(7, out)
SLOT(6, dst)
SLOT(5, out_boxes)
SLOT(4, q)
SLOT(3, conv.output)
SLOT(2, dw.output)
SLOT(1, rz.output)
#undef SLOT

constexpr int kMembers = 3;

template <class P>
void Mark(P& p, uintptr_t tag) {
  auto& slot = Slot(p, Rank<8>{});
  slot = reinterpret_cast<std::remove_reference_t<decltype(slot)>>(tag);
}
void Mark(ConvGroupArgs& p, uintptr_t tag) {
  for (int i = 0; i < kMembers; ++i) {
    bh_conv_params c{};
    c.output = reinterpret_cast<void*>(tag + i);
    p.members.push_back(c);
  }
  p.cgroup.n = kMembers;
}
void Mark(LayerNormArgs& p, uintptr_t tag) {
  auto block = std::make_shared<bh_layernorm_params>();
  block->output = reinterpret_cast<void*>(tag);
  p.p = std::move(block);
}

template <class P>
bool Marked(const P& p, uintptr_t tag) {
  return reinterpret_cast<uintptr_t>(Slot(p, Rank<8>{})) == tag;
}
bool Marked(const ConvGroupArgs& p, uintptr_t tag) {
  if (p.members.size() != kMembers || p.cgroup.n != kMembers) return false;
  for (int i = 0; i < kMembers; ++i)
    if (reinterpret_cast<uintptr_t>(p.members[i].output) != tag + i) return false;
  return true;
}
bool Marked(const LayerNormArgs& p, uintptr_t tag) { return p.p && reinterpret_cast<uintptr_t>(p.p->output) == tag; }

// the pointer accessor of alternative I answers exactly when the launch holds it
template <size_t I>
void CheckAccessor(const Launch& l, size_t held) {
  using Q = std::variant_alternative_t<I, Launch::Payload>;
  CHECK((l.get_if<Q>() != nullptr) == (I == held), l.kind());
}
template <size_t... I>
void CheckAccessors(const Launch& l, size_t held, std::index_sequence<I...>) {
  (CheckAccessor<I>(l, held), ...);
}

template <Launch::Kind K>
void CheckHolds(const Launch& l, uintptr_t tag) {
  using P = Launch::PayloadOf<K>;
  CHECK(l.kind() == K, K);
  const P* p = l.get_if<P>();
  CHECK(p && Marked(*p, tag), K);
  CheckAccessors(l, Launch::kIndex<P>, std::make_index_sequence<std::variant_size_v<Launch::Payload>>{});
  const bool is_conv = K == Launch::kConv || K == Launch::kConvGrouped;
  CHECK((l.conv_if() != nullptr) == is_conv, K);
  if (is_conv && l.conv_if()) {
    CHECK(reinterpret_cast<uintptr_t>(l.conv_if()->output) == tag, K);
    CHECK(&l.conv() == l.conv_if(), K);
  }
}

template <Launch::Kind K>
void CheckKind() {
  using P = Launch::PayloadOf<K>;
  const uintptr_t tag = 0x1000 + 16 * static_cast<uintptr_t>(K);
  P payload{};
  Mark(payload, tag);
  Launch l;
  l.op_index = K;
  l.kernel = "launch_test";
  P& stored = l.Set<K>(payload);
  CHECK(&stored == l.get_if<P>(), K);
  CheckHolds<K>(l, tag);
  // the kind given at run time: the same launch
  Launch r;
  r.Set(K, payload);
  CheckHolds<K>(r, tag);
  // a copy, an assignment over another payload, a move
  Launch c = l;
  CheckHolds<K>(c, tag);
  CheckHolds<K>(l, tag);
  Launch a;
  a.Set<Launch::kCopy>({nullptr, nullptr, 1});
  a = l;
  CheckHolds<K>(a, tag);
  Launch m = std::move(c);
  CheckHolds<K>(m, tag);
  CHECK(m.op_index == K, K);
}

template <int... K>
void CheckKinds(std::integer_sequence<int, K...>) {
  (CheckKind<static_cast<Launch::Kind>(K)>(), ...);
}

}  // namespace

int main() {
  // no payload yet: no runnable kind, every accessor null
  Launch none;
  CHECK(none.kind() == Launch::kNone, Launch::kNone);
  CheckAccessors(none, 0, std::make_index_sequence<std::variant_size_v<Launch::Payload>>{});
  CHECK(none.conv_if() == nullptr, Launch::kNone);

  CheckKinds(std::make_integer_sequence<int, Launch::kNumKinds>{});

  // a new payload replaces the old one (FuseGlue turns a kArgMinMax launch into kResizeArgMinMax)
  Launch l;
  l.Set<Launch::kArgMinMax>().outer = 7;
  l.Set<Launch::kResizeArgMinMax>().out_bytes = 4;
  CHECK(l.kind() == Launch::kResizeArgMinMax, l.kind());
  CHECK(l.get_if<bh_argminmax_params>() == nullptr, l.kind());
  CHECK(l.get_if<bh_resize_argminmax_params>() && l.get_if<bh_resize_argminmax_params>()->out_bytes == 4, l.kind());

  std::printf("%d kinds, sizeof(Launch) %zu: %s\n", static_cast<int>(Launch::kNumKinds), sizeof(Launch),
              g_failed ? "FAILED" : "ok");
  return g_failed ? 1 : 0;
}
