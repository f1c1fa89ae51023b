// The kernel form of a fused depthwise -> 1x1 [-> 1x1] chain as a value: the
// candidate list the tuner (FuseChains, fusion.cc) times, the forms
// BAND_HIP_FUSION=force* pins, and the integer a decision is cached and
// persisted under (BAND_HIP_TUNE_FILE).  Plain host C++ over bh_chain_params.
#pragma once

#include "band_hip_kernels.h"

namespace band {
namespace hip {

struct ChainForm {
  int launches;  // 0: keep the unfused launches; 3: depthwise and both 1x1; 2: the second 1x1 stays a launch
  int px_blocks, waves, persist, tile, deep, c_split, stage;  // bh_chain_params' fields of these names
  int dense = 0;                                               // and this one (last, so seven-field forms read as before)
};
constexpr bool operator==(const ChainForm& a, const ChainForm& b) {
  return a.launches == b.launches && a.px_blocks == b.px_blocks && a.waves == b.waves && a.persist == b.persist &&
         a.tile == b.tile && a.deep == b.deep && a.c_split == b.c_split && a.stage == b.stage && a.dense == b.dense;
}
constexpr ChainForm kUnfused{};
constexpr ChainForm kPlainChain{3, 4, 4, 0, 0, 0, 0, 0};

// The candidates in the order the tuner times them (ties and the 2 % margin
// make the order part of the decision), each written as its 3-launch form.
constexpr ChainForm kChainForms[] = {
    // stage forms (stage 2: loader waves); c_split = phase-C slices
    {3, 1, 4, 0, 0, 0, 0, 1}, {3, 1, 8, 0, 0, 0, 0, 1}, {3, 2, 4, 0, 0, 0, 0, 1}, {3, 2, 8, 0, 0, 0, 0, 1},
    {3, 1, 8, 0, 0, 0, 2, 1}, {3, 2, 8, 0, 0, 0, 2, 1}, {3, 1, 8, 0, 0, 0, 4, 1}, {3, 1, 8, 0, 0, 0, 8, 1},
    {3, 1, 8, 0, 0, 0, 0, 2}, {3, 2, 8, 0, 0, 0, 0, 2}, {3, 1, 4, 0, 0, 0, 0, 2}, {3, 1, 8, 0, 0, 0, 2, 2},
    {3, 2, 8, 0, 0, 0, 2, 2}, {3, 1, 8, 0, 0, 0, 3, 2}, {3, 1, 8, 0, 0, 0, 4, 2}, {3, 1, 8, 0, 0, 0, 8, 2},
    // raster forms: 64 / 32 / 16 pixels per 4-wave workgroup, 16 pixels over
    // 8 / 16 waves (few-pixel, many-channel layers)
    {3, 4, 4, 0, 0, 0, 0, 0}, {3, 2, 4, 0, 0, 0, 0, 0}, {3, 1, 4, 0, 0, 0, 0, 0}, {3, 1, 8, 0, 0, 0, 0, 0},
    {3, 1, 16, 0, 0, 0, 0, 0},
    // persistent form (filters in LDS, 64-pixel blocks walked by one wave of
    // workgroups); 2-D tile form (8 x 8 pixels, one LDS-DMA burst; 3 / 4: runs
    // of 2 / 4 tiles per workgroup, the constant block staged once per run)
    {3, 4, 4, 1, 0, 0, 0, 0}, {3, 4, 4, 0, 1, 0, 0, 0}, {3, 4, 4, 0, 3, 0, 0, 0}, {3, 4, 4, 0, 4, 0, 0, 0},
    // deep-issue raster forms
    {3, 2, 4, 0, 0, 1, 0, 0}, {3, 1, 4, 0, 0, 1, 0, 0}, {3, 1, 8, 0, 0, 1, 0, 0},
    // the second 1x1's channel tiles over 2 .. 4 workgroups per pixel block
    {3, 1, 4, 0, 0, 0, 2, 0}, {3, 1, 8, 0, 0, 0, 2, 0}, {3, 2, 4, 0, 0, 0, 2, 0}, {3, 1, 16, 0, 0, 0, 2, 0},
    {3, 1, 4, 0, 0, 0, 3, 0}, {3, 1, 8, 0, 0, 0, 3, 0}, {3, 1, 4, 0, 0, 0, 4, 0}};

// The dense raster form (chain_dense_kernel: 64 pixels per 4-wave workgroup,
// 8 waves per SIMD, no barrier between the phases), for chains whose grid
// gives every CU several workgroups.  Timed after kChainForms, so a chain
// moves to it only where it beats every earlier form by the tuner's margin;
// a list of its own because the persisted codes and the timing order of
// kChainForms are pinned row by row (tests/native/chain_form_test.cc).
constexpr ChainForm kDenseChainForms[] = {{3, 4, 4, 0, 0, 0, 0, 0, 1}};

// fn(form) for every candidate, in timing order
template <typename Fn>
inline void ForEachChainForm(Fn&& fn) {
  for (const ChainForm& f : kChainForms) fn(f);
  for (const ChainForm& f : kDenseChainForms) fn(f);
}

// Each candidate is timed with 3 launches, then with 2; the stage forms and a
// split of the second 1x1 exist only where the chain holds that 1x1.
constexpr bool HasLaunches(const ChainForm& f, int launches) {
  return launches == 3 || (launches == 2 && !f.stage && f.c_split <= 1);
}
// BAND_HIP_FUSION=notile / nodeep / nosplit / nostage: forms the tuner leaves out
constexpr bool FilteredOut(const ChainForm& f, bool no_tile, bool no_deep, bool no_split, bool no_stage) {
  return f.stage ? no_stage : (f.tile && no_tile) || (f.deep && no_deep) || (f.c_split && no_split);
}

// The persisted integer, whose layout only this function knows.  0: unfused.
// Raster / tile forms: px_blocks, +10 for 2 launches, +100 for 16 waves, +300
// for 8 waves, +200 for the persistent form, +400 / +600 / +700 for tile 1 /
// 3 / 4, +1000 for the deep-issue form, +2000 x (s - 1) for the s-way split
// (s <= 4), +8000 for the dense form (8004 / 8014).
// Stage forms: 100000 + 1000 x (stage - 1) + 100 x slices + 10 x px_blocks +
// (1 for 8 waves).
constexpr int Encode(const ChainForm& f) {
  if (f.launches == 0) return 0;
  if (f.stage) return 100000 + 1000 * (f.stage - 1) + 100 * f.c_split + 10 * f.px_blocks + (f.waves == 8 ? 1 : 0);
  return f.px_blocks + (f.launches == 2 ? 10 : 0) + (f.waves == 16 ? 100 : 0) + (f.waves == 8 ? 300 : 0) +
         (f.persist ? 200 : 0) + (f.tile == 1 ? 400 : 0) + (f.tile == 3 ? 600 : 0) + (f.tile == 4 ? 700 : 0) +
         (f.deep ? 1000 : 0) + (f.c_split > 1 ? 2000 * (f.c_split - 1) : 0) + (f.dense ? 8000 : 0);
}
// false: no candidate (the forced forms are among them) encodes to `code` -
// a tune file of another kernel tree; the caller keeps the unfused launches
inline bool Decode(int code, ChainForm* out) {
  *out = kUnfused;
  if (code == 0) return true;
  bool found = false;
  ForEachChainForm([&](ChainForm f) {
    for (f.launches = 3; f.launches >= 2 && !found; --f.launches)
      if (HasLaunches(f, f.launches) && Encode(f) == code) {
        *out = f;
        found = true;
      }
  });
  return found;
}

inline void Apply(const ChainForm& f, bh_chain_params* q) {
  q->px_blocks = f.px_blocks;
  q->waves = f.waves;
  q->persist = f.persist;
  q->tile = f.tile;
  q->deep = f.deep;
  q->c_split = f.c_split;
  q->stage = f.stage;
  q->dense = f.dense;
}
inline bool Fits(ChainForm f, bh_chain_params q) {
  Apply(f, &q);
  return bh_chain_lds_bytes(&q) > 0;
}

// BAND_HIP_FUSION=forcechain / forcetile / forcedeep / forcestage /
// forcedense (parity tests): the chain `q` (with or without its second 1x1)
// in the named form where that fits, else in the plain one.
enum class ForcedChain { kNone, kPlain, kTile, kDeep, kStage, kDense };
inline ChainForm ForcedForm(ForcedChain kind, const bh_chain_params& q) {
  ChainForm plain = kPlainChain, want = kPlainChain;
  plain.launches = want.launches = q.has_pw2 ? 3 : 2;
  if (kind == ForcedChain::kTile) want.tile = 1;
  if (kind == ForcedChain::kDeep) want.px_blocks = want.deep = 1;
  if (kind == ForcedChain::kDense) want.dense = 1;
  if (kind == ForcedChain::kStage && q.has_pw2) {  // 1 block, 8 waves, 2 slices; with loader waves where they fit too
    want = ChainForm{3, 1, 8, 0, 0, 0, 2, 1};
    ChainForm loader = want;
    loader.stage = 2;
    if (Fits(want, q) && Fits(loader, q)) want = loader;
  }
  return Fits(want, q) ? want : plain;
}

}  // namespace hip
}  // namespace band
