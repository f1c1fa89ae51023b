// Host-only unit test of backend/hip/chain_form.h with the dense raster form
// beside the candidates of kChainForms: every candidate the tuner times, with
// 3 and with 2 launches, persists as an integer of its own and decodes back;
// the integers of the forms that existed before the dense form are the ones
// listed here.
//   g++ -std=c++17 -Iinclude -Iband_amd/csrc tests/native/chain_form_dense_test.cc
#include "backend/hip/chain_form.h"

#include <cstdio>
#include <iterator>
#include <set>
#include <vector>

using namespace band::hip;

// the kernel library's gate, stood in for: the dense form fits unless refused
static bool g_refuse_dense = false;
extern "C" size_t bh_chain_lds_bytes(const bh_chain_params* p) { return p->dense && g_refuse_dense ? 0 : 1024; }

static int g_failures = 0;
#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      ++g_failures;                                               \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                             \
  } while (0)

// code -> {launches, px_blocks, waves, persist, tile, deep, c_split, stage}
struct Row {
  int code;
  ChainForm form;
};
static const Row kBefore[] = {
    {0, {0, 0, 0, 0, 0, 0, 0, 0}},        {1, {3, 1, 4, 0, 0, 0, 0, 0}},        {2, {3, 2, 4, 0, 0, 0, 0, 0}},
    {4, {3, 4, 4, 0, 0, 0, 0, 0}},        {11, {2, 1, 4, 0, 0, 0, 0, 0}},       {12, {2, 2, 4, 0, 0, 0, 0, 0}},
    {14, {2, 4, 4, 0, 0, 0, 0, 0}},       {101, {3, 1, 16, 0, 0, 0, 0, 0}},     {111, {2, 1, 16, 0, 0, 0, 0, 0}},
    {204, {3, 4, 4, 1, 0, 0, 0, 0}},      {214, {2, 4, 4, 1, 0, 0, 0, 0}},      {301, {3, 1, 8, 0, 0, 0, 0, 0}},
    {311, {2, 1, 8, 0, 0, 0, 0, 0}},      {404, {3, 4, 4, 0, 1, 0, 0, 0}},      {414, {2, 4, 4, 0, 1, 0, 0, 0}},
    {604, {3, 4, 4, 0, 3, 0, 0, 0}},      {614, {2, 4, 4, 0, 3, 0, 0, 0}},      {704, {3, 4, 4, 0, 4, 0, 0, 0}},
    {714, {2, 4, 4, 0, 4, 0, 0, 0}},      {1001, {3, 1, 4, 0, 0, 1, 0, 0}},     {1002, {3, 2, 4, 0, 0, 1, 0, 0}},
    {1011, {2, 1, 4, 0, 0, 1, 0, 0}},     {1012, {2, 2, 4, 0, 0, 1, 0, 0}},     {1301, {3, 1, 8, 0, 0, 1, 0, 0}},
    {1311, {2, 1, 8, 0, 0, 1, 0, 0}},     {2001, {3, 1, 4, 0, 0, 0, 2, 0}},     {2002, {3, 2, 4, 0, 0, 0, 2, 0}},
    {2101, {3, 1, 16, 0, 0, 0, 2, 0}},    {2301, {3, 1, 8, 0, 0, 0, 2, 0}},     {4001, {3, 1, 4, 0, 0, 0, 3, 0}},
    {4301, {3, 1, 8, 0, 0, 0, 3, 0}},     {6001, {3, 1, 4, 0, 0, 0, 4, 0}},     {100010, {3, 1, 4, 0, 0, 0, 0, 1}},
    {100011, {3, 1, 8, 0, 0, 0, 0, 1}},   {100020, {3, 2, 4, 0, 0, 0, 0, 1}},   {100021, {3, 2, 8, 0, 0, 0, 0, 1}},
    {100211, {3, 1, 8, 0, 0, 0, 2, 1}},   {100221, {3, 2, 8, 0, 0, 0, 2, 1}},   {100411, {3, 1, 8, 0, 0, 0, 4, 1}},
    {100811, {3, 1, 8, 0, 0, 0, 8, 1}},   {101010, {3, 1, 4, 0, 0, 0, 0, 2}},   {101011, {3, 1, 8, 0, 0, 0, 0, 2}},
    {101021, {3, 2, 8, 0, 0, 0, 0, 2}},   {101211, {3, 1, 8, 0, 0, 0, 2, 2}},   {101221, {3, 2, 8, 0, 0, 0, 2, 2}},
    {101311, {3, 1, 8, 0, 0, 0, 3, 2}},   {101411, {3, 1, 8, 0, 0, 0, 4, 2}},   {101811, {3, 1, 8, 0, 0, 0, 8, 2}},
};

int main() {
  // every candidate, with 3 and 2 launches: one integer each, and back
  std::vector<ChainForm> all;
  ForEachChainForm([&](ChainForm f) {
    for (int launches : {3, 2}) {
      f.launches = launches;
      if (HasLaunches(f, launches)) all.push_back(f);
    }
  });
  CHECK(all.size() == (std::size(kChainForms) + std::size(kDenseChainForms)) * 2 - 16 - 7);  // 16 stage, 7 split rows: 3 only
  std::set<int> codes = {0};
  for (const ChainForm& f : all) {
    ChainForm back{};
    CHECK(Encode(f) != 0);
    CHECK(codes.insert(Encode(f)).second);
    CHECK(Decode(Encode(f), &back) && back == f);
  }
  // the forms that existed before: the same integers, and none of them dense
  for (const Row& r : kBefore) {
    ChainForm f{};
    CHECK(Encode(r.form) == r.code);
    CHECK(Decode(r.code, &f) && f == r.form && f.dense == 0);
    CHECK(codes.count(r.code) == 1);
  }
  // the dense form: 8004 / 8014, between the raster codes' 7,714 ceiling and 10,000
  CHECK(codes.size() == std::size(kBefore) + 2);
  const ChainForm dense3{3, 4, 4, 0, 0, 0, 0, 0, 1}, dense2{2, 4, 4, 0, 0, 0, 0, 0, 1};
  CHECK(Encode(dense3) == 8004 && Encode(dense2) == 8014);
  ChainForm f{};
  CHECK(Decode(8004, &f) && f == dense3);
  CHECK(Decode(8014, &f) && f == dense2);
  for (int bad : {8001, 8002, 8024, 8104, 8204, 8404, 9004, 10004, 16004, 108004}) CHECK(!Decode(bad, &f));
  CHECK(!(dense3 == kPlainChain));
  // it is timed last, with 3 launches and with 2, and no filter of the tuner drops it
  CHECK(all.back() == dense2 && all[all.size() - 2] == dense3);
  CHECK(!FilteredOut(dense3, true, true, true, true));
  // Apply writes the field; a seven-field form clears it
  bh_chain_params q{};
  Apply(dense3, &q);
  CHECK(q.dense == 1 && q.px_blocks == 4 && q.waves == 4 && !q.persist && !q.tile && !q.deep && !q.c_split && !q.stage);
  Apply(ChainForm{3, 1, 8, 0, 0, 0, 3, 2}, &q);
  CHECK(q.dense == 0 && q.stage == 2);
  // forcedense: the dense form where it fits, else plain; with and without a second 1x1
  bh_chain_params with{}, without{};
  with.has_pw2 = 1;
  CHECK(Encode(ForcedForm(ForcedChain::kDense, with)) == 8004 && Encode(ForcedForm(ForcedChain::kDense, without)) == 8014);
  g_refuse_dense = true;
  CHECK(Encode(ForcedForm(ForcedChain::kDense, with)) == 4 && Encode(ForcedForm(ForcedChain::kDense, without)) == 14);
  CHECK(!Fits(dense3, with) && Fits(kPlainChain, with));
  g_refuse_dense = false;
  std::printf("%d failures\n", g_failures);
  return g_failures ? 1 : 0;
}
