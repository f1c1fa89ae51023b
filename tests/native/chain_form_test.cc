// Host-only unit test of backend/hip/chain_form.h: the chain tuner's form
// descriptor and the integer it is persisted as (BAND_HIP_TUNE_FILE).
//   g++ -std=c++17 -Iinclude -Iband_amd/csrc tests/native/chain_form_test.cc
#include "backend/hip/chain_form.h"

#include <cstdio>
#include <iterator>
#include <set>
#include <vector>

using namespace band::hip;

// The kernel library's gate, stood in for: a form fits unless it is a tile /
// deep / stage-1 / stage-2 form and the matching bit of g_refuse is set.
enum { kNoTile = 1, kNoDeep = 2, kNoStage1 = 4, kNoStage2 = 8 };
static int g_refuse = 0;
extern "C" size_t bh_chain_lds_bytes(const bh_chain_params* p) {
  if ((p->tile && (g_refuse & kNoTile)) || (p->deep && (g_refuse & kNoDeep)) ||
      (p->stage == 1 && (g_refuse & kNoStage1)) || (p->stage == 2 && (g_refuse & kNoStage2)))
    return 0;
  return 1024;
}

static int g_failures = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      ++g_failures;                                                         \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);           \
    }                                                                       \
  } while (0)

// code -> {launches, px_blocks, waves, persist, tile, deep, c_split, stage}
// as the decode arithmetic FuseChains carried before chain_form.h read it:
// every integer the candidate list or a forced form yields, which covers
// every integer of profiles/r06an_tune.tsv and r06i / r06n / r06s_tune.txt.
struct Row {
  int code;
  ChainForm form;
};
static const Row kTable[] = {
    {0, {0, 0, 0, 0, 0, 0, 0, 0}},
    {1, {3, 1, 4, 0, 0, 0, 0, 0}},
    {2, {3, 2, 4, 0, 0, 0, 0, 0}},
    {4, {3, 4, 4, 0, 0, 0, 0, 0}},
    {11, {2, 1, 4, 0, 0, 0, 0, 0}},
    {12, {2, 2, 4, 0, 0, 0, 0, 0}},
    {14, {2, 4, 4, 0, 0, 0, 0, 0}},
    {101, {3, 1, 16, 0, 0, 0, 0, 0}},
    {111, {2, 1, 16, 0, 0, 0, 0, 0}},
    {204, {3, 4, 4, 1, 0, 0, 0, 0}},
    {214, {2, 4, 4, 1, 0, 0, 0, 0}},
    {301, {3, 1, 8, 0, 0, 0, 0, 0}},
    {311, {2, 1, 8, 0, 0, 0, 0, 0}},
    {404, {3, 4, 4, 0, 1, 0, 0, 0}},
    {414, {2, 4, 4, 0, 1, 0, 0, 0}},
    {604, {3, 4, 4, 0, 3, 0, 0, 0}},
    {614, {2, 4, 4, 0, 3, 0, 0, 0}},
    {704, {3, 4, 4, 0, 4, 0, 0, 0}},
    {714, {2, 4, 4, 0, 4, 0, 0, 0}},
    {1001, {3, 1, 4, 0, 0, 1, 0, 0}},
    {1002, {3, 2, 4, 0, 0, 1, 0, 0}},
    {1011, {2, 1, 4, 0, 0, 1, 0, 0}},
    {1012, {2, 2, 4, 0, 0, 1, 0, 0}},
    {1301, {3, 1, 8, 0, 0, 1, 0, 0}},
    {1311, {2, 1, 8, 0, 0, 1, 0, 0}},
    {2001, {3, 1, 4, 0, 0, 0, 2, 0}},
    {2002, {3, 2, 4, 0, 0, 0, 2, 0}},
    {2101, {3, 1, 16, 0, 0, 0, 2, 0}},
    {2301, {3, 1, 8, 0, 0, 0, 2, 0}},
    {4001, {3, 1, 4, 0, 0, 0, 3, 0}},
    {4301, {3, 1, 8, 0, 0, 0, 3, 0}},
    {6001, {3, 1, 4, 0, 0, 0, 4, 0}},
    {100010, {3, 1, 4, 0, 0, 0, 0, 1}},
    {100011, {3, 1, 8, 0, 0, 0, 0, 1}},
    {100020, {3, 2, 4, 0, 0, 0, 0, 1}},
    {100021, {3, 2, 8, 0, 0, 0, 0, 1}},
    {100211, {3, 1, 8, 0, 0, 0, 2, 1}},
    {100221, {3, 2, 8, 0, 0, 0, 2, 1}},
    {100411, {3, 1, 8, 0, 0, 0, 4, 1}},
    {100811, {3, 1, 8, 0, 0, 0, 8, 1}},
    {101010, {3, 1, 4, 0, 0, 0, 0, 2}},
    {101011, {3, 1, 8, 0, 0, 0, 0, 2}},
    {101021, {3, 2, 8, 0, 0, 0, 0, 2}},
    {101211, {3, 1, 8, 0, 0, 0, 2, 2}},
    {101221, {3, 2, 8, 0, 0, 0, 2, 2}},
    {101311, {3, 1, 8, 0, 0, 0, 3, 2}},
    {101411, {3, 1, 8, 0, 0, 0, 4, 2}},
    {101811, {3, 1, 8, 0, 0, 0, 8, 2}},
};

// the candidates in timing order as {px_blocks, waves, persist, tile, deep,
// c_split, stage}: the 16 stage forms, then the 19 raster / tile / deep /
// split rows
static const int kOrder[][7] = {
    {1, 4, 0, 0, 0, 0, 1}, {1, 8, 0, 0, 0, 0, 1}, {2, 4, 0, 0, 0, 0, 1}, {2, 8, 0, 0, 0, 0, 1}, {1, 8, 0, 0, 0, 2, 1},
    {2, 8, 0, 0, 0, 2, 1}, {1, 8, 0, 0, 0, 4, 1}, {1, 8, 0, 0, 0, 8, 1}, {1, 8, 0, 0, 0, 0, 2}, {2, 8, 0, 0, 0, 0, 2},
    {1, 4, 0, 0, 0, 0, 2}, {1, 8, 0, 0, 0, 2, 2}, {2, 8, 0, 0, 0, 2, 2}, {1, 8, 0, 0, 0, 3, 2}, {1, 8, 0, 0, 0, 4, 2},
    {1, 8, 0, 0, 0, 8, 2},
    {4, 4, 0, 0, 0, 0, 0}, {2, 4, 0, 0, 0, 0, 0}, {1, 4, 0, 0, 0, 0, 0}, {1, 8, 0, 0, 0, 0, 0}, {1, 16, 0, 0, 0, 0, 0},
    {4, 4, 1, 0, 0, 0, 0}, {4, 4, 0, 1, 0, 0, 0}, {4, 4, 0, 3, 0, 0, 0}, {4, 4, 0, 4, 0, 0, 0}, {2, 4, 0, 0, 1, 0, 0},
    {1, 4, 0, 0, 1, 0, 0}, {1, 8, 0, 0, 1, 0, 0}, {1, 4, 0, 0, 0, 2, 0}, {1, 8, 0, 0, 0, 2, 0}, {2, 4, 0, 0, 0, 2, 0},
    {1, 16, 0, 0, 0, 2, 0}, {1, 4, 0, 0, 0, 3, 0}, {1, 8, 0, 0, 0, 3, 0}, {1, 4, 0, 0, 0, 4, 0}};

// every form the tuner can time or a force* value can pin, plus "unfused"
static std::vector<ChainForm> AllForms() {
  std::vector<ChainForm> all = {kUnfused};
  for (ChainForm f : kChainForms)
    for (int launches : {3, 2}) {
      f.launches = launches;
      if (HasLaunches(f, launches)) all.push_back(f);
    }
  bh_chain_params with{}, without{};
  with.has_pw2 = 1;
  for (int refuse = 0; refuse < 16; ++refuse) {
    g_refuse = refuse;
    for (ForcedChain k : {ForcedChain::kPlain, ForcedChain::kTile, ForcedChain::kDeep, ForcedChain::kStage})
      for (const bh_chain_params* q : {&with, &without}) all.push_back(ForcedForm(k, *q));
  }
  g_refuse = 0;
  return all;
}

static int ForcedCode(ForcedChain k, int has_pw2, int refuse) {
  bh_chain_params q{};
  q.has_pw2 = has_pw2;
  g_refuse = refuse;
  const int code = Encode(ForcedForm(k, q));
  g_refuse = 0;
  return code;
}

int main() {
  // round trip, and one integer per form
  std::set<int> codes;
  std::vector<ChainForm> seen;
  for (const ChainForm& f : AllForms()) {
    ChainForm back{};
    CHECK(Decode(Encode(f), &back) && back == f);
    bool known = false;
    for (const ChainForm& s : seen) known = known || s == f;
    if (known) continue;
    seen.push_back(f);
    CHECK(codes.insert(Encode(f)).second);
  }
  // the integers and their meaning are those of the table, no more, no fewer
  CHECK(codes.size() == std::size(kTable));
  for (const Row& r : kTable) {
    ChainForm f{};
    CHECK(codes.count(r.code) == 1);
    CHECK(Decode(r.code, &f) && f == r.form);
    CHECK(Encode(r.form) == r.code);
  }
  for (int bad : {5, 24, 401, 1004, 4002, 8001, 99999, 100000, 100012, 100110, 102011, -1}) {
    ChainForm f{};
    CHECK(!Decode(bad, &f));
  }
  // timing order
  CHECK(std::size(kChainForms) == std::size(kOrder));
  for (size_t i = 0; i < std::size(kChainForms) && i < std::size(kOrder); ++i) {
    const int* o = kOrder[i];
    CHECK((kChainForms[i] == ChainForm{3, o[0], o[1], o[2], o[3], o[4], o[5], o[6]}));
  }
  // which launch counts a row is timed with, and the tuner's filters
  for (const ChainForm& f : kChainForms) {
    CHECK(HasLaunches(f, 3));
    CHECK(HasLaunches(f, 2) == (!f.stage && f.c_split <= 1));
    CHECK(!FilteredOut(f, false, false, false, false));
    CHECK(FilteredOut(f, true, false, false, false) == (f.tile != 0));
    CHECK(FilteredOut(f, false, true, false, false) == (f.deep != 0));
    CHECK(FilteredOut(f, false, false, true, false) == (!f.stage && f.c_split != 0));
    CHECK(FilteredOut(f, false, false, false, true) == (f.stage != 0));
  }
  // forced forms: the preferred one where it fits, else plain px 4 / 4 waves
  CHECK(ForcedCode(ForcedChain::kPlain, 1, 0) == 4 && ForcedCode(ForcedChain::kPlain, 0, 0) == 14);
  CHECK(ForcedCode(ForcedChain::kTile, 1, 0) == 404 && ForcedCode(ForcedChain::kTile, 0, 0) == 414);
  CHECK(ForcedCode(ForcedChain::kTile, 1, kNoTile) == 4 && ForcedCode(ForcedChain::kTile, 0, kNoTile) == 14);
  CHECK(ForcedCode(ForcedChain::kDeep, 1, 0) == 1001 && ForcedCode(ForcedChain::kDeep, 0, 0) == 1011);
  CHECK(ForcedCode(ForcedChain::kDeep, 1, kNoDeep) == 4 && ForcedCode(ForcedChain::kDeep, 0, kNoDeep) == 14);
  CHECK(ForcedCode(ForcedChain::kStage, 1, 0) == 101211 && ForcedCode(ForcedChain::kStage, 1, kNoStage2) == 100211);
  CHECK(ForcedCode(ForcedChain::kStage, 1, kNoStage1) == 4 && ForcedCode(ForcedChain::kStage, 1, kNoStage1 | kNoStage2) == 4);
  CHECK(ForcedCode(ForcedChain::kStage, 0, 0) == 14);  // no second 1x1: the plain 2-launch form
  // Apply writes the seven form fields and nothing else
  bh_chain_params q{};
  q.has_pw2 = 7;
  Apply(ChainForm{3, 1, 8, 0, 0, 0, 3, 2}, &q);
  CHECK(q.px_blocks == 1 && q.waves == 8 && q.persist == 0 && q.tile == 0 && q.deep == 0 && q.c_split == 3 &&
        q.stage == 2 && q.has_pw2 == 7);
  Apply(ChainForm{2, 4, 4, 1, 4, 1, 0, 0}, &q);
  CHECK(q.px_blocks == 4 && q.waves == 4 && q.persist == 1 && q.tile == 4 && q.deep == 1 && q.c_split == 0 &&
        q.stage == 0);
  std::printf("%d failures\n", g_failures);
  return g_failures ? 1 : 0;
}
