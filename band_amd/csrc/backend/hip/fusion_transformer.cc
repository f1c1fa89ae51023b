// HipModelExecutor: the fusion passes for transformer blocks (kGPU; the
// privacy rule and DropDead are fusion.cc's).  MatchLayerNorm and FuseTenOps
// serve FuseLayerNorm (int8) and FuseLayerNormF32 (opt-in), FoldLayerNormQuant
// folds the hybrid FULLY_CONNECTEDs' row quantisation into the float32 launch,
// FuseAttention (opt-in) makes the int8 attention core one launch.
#include "backend/hip/executor_internal.h"

namespace band {
namespace hip {

using namespace ex;

// The ten ops a converter makes of a LayerNormalization over the last axis,
// in the order and with the operand order the synthesiser emits:
//   m = MEAN(x)  d = SQUARED_DIFFERENCE(x, m)  v = MEAN(d)  e = ADD(v, eps)
//   r = RSQRT(e)  g = MUL(r, gamma)  a = MUL(x, g)  b = MUL(m, g)
//   c = SUB(beta, b)  y = ADD(a, c)
// on x [..., C], one row statistic per row, constants gamma / beta [C] and eps
// of one element.  Op by op that is ten launches at the dispatch floor.
struct LnMatch {
  const TflOperator* o[10];
  int x, m, dd, v, e, r, g, a, b, c, y, eps, gamma, beta;
  long depth;  // C
};

// ls[i .. i+9] are that pattern as launches of `kinds`: each materialises its
// op's one output, the operands are wired as above, y and the per-element
// intermediates have x's shape, the constants theirs, and the nine
// intermediates are PrivateTo the ten ops.  Types, the row statistics' shape
// and the launches' own parameters are the caller's to check.
bool HipModelExecutor::MatchLayerNorm(const TflModel& d, const PreparedSubgraph& sg, const std::vector<Launch>& ls,
                                      size_t i, const Launch::Kind kinds[10], LnMatch* n) const {
  static const int kPattern[10] = {kTflMean, kTflSquaredDifference, kTflMean, kTflAdd, kTflRsqrt,
                                   kTflMul,  kTflMul,               kTflMul,  kTflSub, kTflAdd};
  if (i + 10 > ls.size()) return false;
  std::set<int> inside;
  for (int k = 0; k < 10; ++k) {
    const Launch& l = ls[i + k];
    if (l.kind() != kinds[k] || l.op_index < 0) return false;
    const TflOperator& op = d.ops[l.op_index];
    if (op.builtin != kPattern[k] || op.outputs.size() != 1 || l.out_tensor != op.outputs[0] ||
        op.inputs.size() < (k == 4 ? 1u : 2u))
      return false;
    n->o[k] = &op;
    inside.insert(l.op_index);
  }
  auto in = [&](int k, int j) { return n->o[k]->inputs[j]; };
  auto res = [&](int k) { return n->o[k]->outputs[0]; };
  const int x = in(0, 0), m = res(0), dd = res(1), v = res(2), e = res(3), r = res(4), g = res(5), a = res(6),
            b = res(7), c = res(8), y = res(9), eps = in(3, 1), gamma = in(5, 1), beta = in(8, 0);
  if (x < 0 || in(1, 0) != x || in(1, 1) != m || in(2, 0) != dd || in(3, 0) != v || in(4, 0) != e || in(5, 0) != r ||
      in(6, 0) != x || in(6, 1) != g || in(7, 0) != m || in(7, 1) != g || in(8, 1) != b || in(9, 0) != a ||
      in(9, 1) != c || eps < 0 || gamma < 0 || beta < 0)
    return false;
  const TflTensor& tx = d.tensors[x];
  const long depth = !tx.shape.empty() ? tx.shape.back() : 0;
  const std::vector<int> per_channel = {static_cast<int>(depth)};
  if (depth < 1 || d.tensors[y].shape != tx.shape || !d.tensors[eps].is_const() || d.tensors[eps].num_elements() != 1 ||
      !d.tensors[gamma].is_const() || d.tensors[gamma].shape != per_channel || !d.tensors[beta].is_const() ||
      d.tensors[beta].shape != per_channel)
    return false;
  for (int t : {dd, g, a, b, c})
    if (d.tensors[t].shape != tx.shape) return false;
  for (int t : {m, dd, v, e, r, g, a, b, c})
    if (!PrivateTo(d, sg, t, inside)) return false;
  n->x = x, n->m = m, n->dd = dd, n->v = v, n->e = e, n->r = r, n->g = g, n->a = a, n->b = b, n->c = c, n->y = y;
  n->eps = eps, n->gamma = gamma, n->beta = beta, n->depth = depth;
  return true;
}

// The loop of both LayerNorm passes.  Where MatchLayerNorm takes ten launches
// and `fill` (the pass's own checks, then *F from the match n and the ten
// launches l[0 .. 9]) agrees, they leave as the one launch *F: ops 1 .. 9 and
// the nine intermediates are gone (a later view of one re-lowers).
void HipModelExecutor::FuseTenOps(const TflModel& d, PreparedSubgraph* sg, const Launch::Kind kinds[10],
                                  const std::function<bool(const LnMatch& n, const Launch* l, Launch* F)>& fill) {
  std::vector<Launch> out;
  const std::vector<Launch>& ls = sg->launches;
  for (size_t i = 0; i < ls.size(); ++i) {
    LnMatch n;
    Launch F;
    if (!MatchLayerNorm(d, *sg, ls, i, kinds, &n) || !fill(n, &ls[i], &F)) {
      out.push_back(ls[i]);
      continue;
    }
    F.op_index = ls[i].op_index;
    F.out_tensor = n.y;
    for (int k = 1; k < 10; ++k) sg->fused_ops.insert(ls[i + k].op_index);
    for (int t : {n.m, n.dd, n.v, n.e, n.r, n.g, n.a, n.b, n.c}) sg->fused_tensors.insert(t);
    out.push_back(F);
    i += 9;
  }
  sg->launches.swap(out);
}

// int8: kMeanRows, kEltwise, kMeanRows, kEltwise, kLutU8 (RSQRT), kEltwise x 5
// become one layernorm_i8_kernel launch that carries the ten parameter blocks
// as they were lowered, so it stores the same bytes.  They qualify when x is
// int8, the row statistics hold one value per row, and the launcher's check
// takes the row (C <= BH_LAYERNORM_MAX_DEPTH).
void HipModelExecutor::FuseLayerNorm(const HipModel& model, PreparedSubgraph* sg) {
  const TflModel& d = model.desc();
  static const Launch::Kind kKinds[10] = {Launch::kMeanRows, Launch::kEltwise, Launch::kMeanRows, Launch::kEltwise,
                                          Launch::kLutU8,    Launch::kEltwise, Launch::kEltwise,  Launch::kEltwise,
                                          Launch::kEltwise,  Launch::kEltwise};
  FuseTenOps(d, sg, kKinds, [&](const LnMatch& n, const Launch* l, Launch* F) {
    const TflTensor& tx = d.tensors[n.x];
    bool ok = tx.type == DataType::kInt8 && d.tensors[n.eps].data_size >= 1;
    for (int t : {n.m, n.v, n.e, n.r})
      ok = ok && d.tensors[t].num_elements() * static_cast<size_t>(n.depth) == tx.num_elements();
    if (!ok) return false;
    auto block = std::make_shared<bh_layernorm_params>();
    bh_layernorm_params& p = *block;
    auto elt = [&](int k) -> const bh_eltwise_params& { return l[k].as<bh_eltwise_params>(); };
    p.mean_x = l[0].as<bh_mean_rows_params>();
    p.rows = p.mean_x.rows;
    p.depth = static_cast<int>(n.depth);
    p.sqdiff = elt(1);
    p.mean_d = l[2].as<bh_mean_rows_params>();
    p.add_eps = elt(3);
    p.rsqrt_table = l[4].as<LutArgs>().table;
    p.mul_gamma = elt(5);
    p.mul_x = elt(6);
    p.mul_m = elt(7);
    p.sub_beta = elt(8);
    p.add_out = elt(9);
    p.eps_q = static_cast<int8_t>(d.tensors[n.eps].data[0]);
    p.input = p.mean_x.input;
    p.gamma = p.mul_gamma.b;
    p.beta = p.sub_beta.a;
    p.output = p.add_out.out;
    if (p.mean_d.rows != p.rows || bh_layernorm_i8_check(&p) != 0) return false;
    F->kernel = bh_layernorm_i8_kernel(&p);
    F->Set<Launch::kLayerNorm>({std::move(block)});
    F->alg_bytes = 2.0 * static_cast<double>(tx.num_elements()) + 2.0 * n.depth + 256.0;
    return true;
  });
}

// float32 (FGraph.layer_norm; BAND_HIP_FUSED_LAYERNORM_F32=1): kMean,
// kEltwiseF32 (SQDIFF), kMean, kEltwiseF32 (ADD), kUnaryF32 (RSQRT),
// kEltwiseF32 x 5 (MUL, MUL, MUL, SUB, ADD) become one layernorm_f32_kernel
// launch.  They qualify when every tensor is float32, the MEANs run over the
// last axis with keep_dims, every fused activation is NONE, eps holds a
// float32 (its value is taken here), and the launcher's check takes the row
// (C <= BH_LAYERNORM_F32_MAX_DEPTH).  The kernel's two row sums have an order
// of their own (band_hip_kernels.h), so its result lies within the ops' error
// bound but is not their bits.
//   A model whose constants are fp16 behind DEQUANTIZE ops lowers a
// DEQUANTIZE launch between the MEAN and the ADD of eps (and its gamma / beta
// are no constants): it never presents the ten consecutive launches and keeps
// them.
void HipModelExecutor::FuseLayerNormF32(const HipModel& model, PreparedSubgraph* sg) {
  const TflModel& d = model.desc();
  static const Launch::Kind kKinds[10] = {Launch::kMean,       Launch::kEltwiseF32, Launch::kMean,       Launch::kEltwiseF32,
                                          Launch::kUnaryF32,   Launch::kEltwiseF32, Launch::kEltwiseF32, Launch::kEltwiseF32,
                                          Launch::kEltwiseF32, Launch::kEltwiseF32};
  static const int kElt[10] = {-1, BH_ELTF_SQDIFF, -1, BH_ELTF_ADD, -1, BH_ELTF_MUL, BH_ELTF_MUL, BH_ELTF_MUL, BH_ELTF_SUB,
                               BH_ELTF_ADD};
  const float inf = std::numeric_limits<float>::infinity();
  FuseTenOps(d, sg, kKinds, [&](const LnMatch& n, const Launch* l, Launch* F) {
    auto eltf = [&](int k) -> const bh_eltwise_f32_params& { return l[k].as<bh_eltwise_f32_params>(); };
    bool ok = l[4].as<UnaryF32Args>().kind == BH_UNARY_RSQRT && d.tensors[n.eps].data_size >= 4;
    for (int k = 0; k < 10; ++k)
      ok = ok && (kElt[k] < 0 || (eltf(k).kind == kElt[k] && eltf(k).act_min == -inf && eltf(k).act_max == inf));
    for (int t : {n.x, n.m, n.dd, n.v, n.e, n.r, n.g, n.a, n.b, n.c, n.y, n.eps, n.gamma, n.beta})
      ok = ok && d.tensors[t].type == DataType::kFloat32;
    // the row statistics keep the input's rank with a last axis of 1 (keep_dims)
    const TflTensor& tx = d.tensors[n.x];
    std::vector<int> stat = tx.shape;
    stat.back() = 1;
    for (int t : {n.m, n.v, n.e, n.r}) ok = ok && d.tensors[t].shape == stat;
    // MEAN over the last axis alone: rows x depth x 1
    for (int k : {0, 2}) {
      const bh_mean_params& q = l[k].as<bh_mean_params>();
      ok = ok && q.type == 0 && q.inner == 1 && q.reduce == n.depth &&
           q.outer * n.depth == static_cast<long>(tx.num_elements());
    }
    if (!ok) return false;
    bh_layernorm_f32_params& p = F->Set<Launch::kLayerNormF32>();
    p.rows = l[0].as<bh_mean_params>().outer;
    p.depth = static_cast<int>(n.depth);
    std::memcpy(&p.eps, d.tensors[n.eps].data, sizeof(float));
    p.input = static_cast<const float*>(l[0].as<bh_mean_params>().input);
    p.gamma = eltf(5).b;
    p.beta = eltf(8).a;
    p.output = eltf(9).out;
    if (eltf(6).a != p.input || bh_layernorm_f32_check(&p) != 0) return false;
    F->kernel = bh_layernorm_f32_kernel(&p);
    F->alg_bytes = 8.0 * static_cast<double>(tx.num_elements()) + 8.0 * n.depth;
    return true;
  });
}

// The row quantisation of the hybrid FULLY_CONNECTEDs that read a fused
// float32 LayerNorm's result y, folded into that launch: the finished row is
// quantised once, in registers, for all of them.  Per fused launch: the
// kDynQuantRows launches whose op reads tensor y itself, over its rows x
// depth, in one form (the first reader's; a reader of the other form keeps its
// launch) are dropped, the fused launch writes q / scale / offset into the
// first one's scratch, and every such op's kFcHybrid block reads that scratch.
// y itself is then stored only when something still reads it: an op whose
// launch was not folded, an output, a view (no_fuse / extra_d2h).  Otherwise
// it joins fused_tensors, so a later view re-lowers with y materialised.
void HipModelExecutor::FoldLayerNormQuant(const HipModel& model, PreparedSubgraph* sg) {
  const TflModel& d = model.desc();
  std::vector<Launch>& ls = sg->launches;
  std::vector<bool> dead(ls.size(), false);
  for (size_t i = 0; i < ls.size(); ++i) {
    bh_layernorm_f32_params* lnf = ls[i].get_if<bh_layernorm_f32_params>();
    if (!lnf || lnf->q) continue;
    bh_layernorm_f32_params& p = *lnf;
    const int y = ls[i].out_tensor;
    std::set<int> folded;  // ops whose quantisation this launch takes over
    const bh_dynquant_params* first = nullptr;
    for (size_t j = i + 1; j < ls.size(); ++j) {
      const Launch& q = ls[j];
      const bh_dynquant_params* dq = q.get_if<bh_dynquant_params>();
      if (!dq || dead[j] || q.op_index < 0) continue;
      const TflOperator& op = d.ops[q.op_index];
      if (op.inputs.empty() || op.inputs[0] != y || dq->input != p.output || dq->rows != p.rows || dq->depth != p.depth)
        continue;
      if (first && (dq->asymmetric != 0) != (first->asymmetric != 0)) continue;
      if (!first) first = dq;
      folded.insert(q.op_index);
      dead[j] = true;
    }
    if (!first) continue;
    p.q = first->q;
    p.scale = first->scale;
    p.offset = first->offset;
    p.asymmetric = first->asymmetric;
    for (Launch& l : ls)
      if (bh_fc_hybrid_params* fch = folded.count(l.op_index) ? l.get_if<bh_fc_hybrid_params>() : nullptr) {
        fch->q = p.q;
        fch->in_scale = p.scale;
        fch->in_offset = p.offset;
      }
    bool needed = KeptOutside(d, *sg, y);
    for (int consumer : consumers_[y]) needed = needed || !folded.count(consumer);
    ls[i].alg_bytes += 1.0 * static_cast<double>(p.rows) * p.depth + 8.0 * p.rows;
    if (!needed) {
      ls[i].alg_bytes -= 4.0 * static_cast<double>(p.rows) * p.depth;
      p.output = nullptr;
      sg->fused_tensors.insert(y);
    }
    if (bh_layernorm_f32_check(&p) == 0) ls[i].kernel = bh_layernorm_f32_kernel(&p);
  }
  DropDead(&ls, dead);
}

// The attention core of a converted int8 block, three consecutive launches
//   scores = BATCH_MATMUL(q, k, adj_y)   p = SOFTMAX(scores)   ctx = BATCH_MATMUL(p, v)
// becomes one attention_i8_kernel launch (BAND_HIP_FUSED_ATTENTION=1, kGPU)
// that carries the three parameter blocks as they were lowered, so it stores
// the same bytes.  They qualify when scores and p are int8, are read only
// inside the pattern (scores by the SOFTMAX, p by the second product as its
// lhs), are no subgraph or model output and are not viewed (no_fuse /
// extra_d2h), the softmax runs over the scores' last axis, the first product
// has a K-contiguous rhs and no adj_x, the second no adjoint, and the
// launcher's check takes the result (keys <= 1024, head_dim, out_dim <= 128).
//   Head TRANSPOSEs.  q, k or v produced by a kReindex launch that is a
// TRANSPOSE leaving the last axis in place, whose output nothing else reads
// and nobody needs materialised, is read through strides from the TRANSPOSE's
// input and that launch is dropped; a TRANSPOSE of the same kind that is
// ctx's only reader is absorbed into the output strides, and the fused launch
// then writes the TRANSPOSE's output tensor.  An operand that cannot be
// absorbed stays the dense tensor it was.
//   The masked pattern.  Four consecutive launches, with an int8 ADD between
// the first product and the SOFTMAX: exactly one ADD operand is the scores
// (either position); the scores and the ADD's output are private to the
// pattern under the same rule.  The other operand, the bias, is int8, a
// constant or a runtime tensor, and is only read, so it need not be private
// (one padding mask feeds every block); after Shape4 it broadcasts to
// [b0, b1, rows, keys], and its strides are 0 for extents of 1.  The fused
// launch (attention_bias_i8_kernel) carries the ADD's block as lowered, and
// the SOFTMAX's table is then the one of the ADD output's scale.
void HipModelExecutor::FuseAttention(const HipModel& model, PreparedSubgraph* sg) {
  const TflModel& d = model.desc();
  std::vector<Launch>& ls = sg->launches;
  std::vector<bool> dead(ls.size(), false);
  // op is a TRANSPOSE of rank 2 .. 4 that leaves the last axis in place
  auto head_perm = [&](const TflOperator& op, std::vector<int64_t>* perm) {
    if (op.builtin != kTflTranspose || op.inputs.size() < 2 || op.inputs[0] < 0 || op.inputs[1] < 0 ||
        op.outputs.size() != 1)
      return false;
    const size_t r = d.tensors[op.inputs[0]].shape.size();
    if (r < 2 || r > 4 || !ConstInts(d.tensors[op.inputs[1]], perm) || perm->size() != r) return false;
    std::vector<bool> seen(r, false);
    for (int64_t p : *perm) {
      if (p < 0 || p >= static_cast<int64_t>(r) || seen[p]) return false;
      seen[p] = true;
    }
    return perm->back() == static_cast<int64_t>(r) - 1;
  };
  auto dense_strides = [](const std::vector<int>& shape) {
    std::vector<int64_t> s(shape.size(), 1);
    for (int k = static_cast<int>(shape.size()) - 2; k >= 0; --k) s[k] = s[k + 1] * shape[k + 1];
    return s;
  };
  // a matrix operand of dims `dm` walked at strides `st`: its batch strides (0 for a dim of 1) and row stride
  auto operand = [](const std::vector<int64_t>& dm, const std::vector<int64_t>& st, int64_t* bstride, int64_t* row) {
    const int r = static_cast<int>(dm.size());
    bstride[0] = bstride[1] = 0;
    for (int k = 0; k < r - 2; ++k) bstride[2 - (r - 2) + k] = dm[k] == 1 ? 0 : st[k];
    *row = st[r - 2];
  };
  // operand tensor t of op `reader`, at `ptr`: when a head TRANSPOSE launch made it for that op alone, the launch
  // (its index) and the strides that read the TRANSPOSE's input instead
  auto absorb_in = [&](size_t before, int t, int reader, const void* ptr, int64_t* bstride, int64_t* row,
                       const void** src) -> int {
    for (size_t j = before; j-- > 0;) {
      const Launch& r = ls[j];
      if (dead[j] || r.kind() != Launch::kReindex || r.as<bh_reindex_params>().output != ptr || r.out_tensor != t) continue;
      const TflOperator& op = d.ops[r.op_index];
      std::vector<int64_t> perm;
      if (!head_perm(op, &perm) || op.outputs[0] != t || !PrivateTensor(d, *sg, t, reader)) return -1;
      const TflTensor& x = d.tensors[op.inputs[0]];
      const std::vector<int64_t> xs = dense_strides(x.shape);
      std::vector<int64_t> dm, st;
      for (int64_t p : perm) {
        dm.push_back(x.shape[p]);
        st.push_back(xs[p]);
      }
      operand(dm, st, bstride, row);
      *src = r.as<bh_reindex_params>().input;
      return static_cast<int>(j);
    }
    return -1;
  };
  for (size_t i = 0; i + 2 < ls.size(); ++i) {
    const Launch& A = ls[i];
    if (A.kind() != Launch::kBatchMatMul) continue;
    // the masked pattern: an int8 ADD of the scores and a bias between the first product and the SOFTMAX
    const size_t e = ls[i + 1].kind() == Launch::kEltwise ? 1 : 0;
    if (i + 2 + e >= ls.size()) continue;
    const Launch* E = e ? &ls[i + 1] : nullptr;
    const Launch &S = ls[i + 1 + e], &B = ls[i + 2 + e];
    if (S.kind() != Launch::kSoftmax || B.kind() != Launch::kBatchMatMul) continue;
    if (A.op_index < 0 || S.op_index < 0 || B.op_index < 0 || (E && E->op_index < 0)) continue;
    const TflOperator &oa = d.ops[A.op_index], &os = d.ops[S.op_index], &ob = d.ops[B.op_index];
    if (oa.builtin != kTflBatchMatMul || os.builtin != kTflSoftmax || ob.builtin != kTflBatchMatMul) continue;
    auto adj = [](const TflOperator& op, int k) { return op.options.valid() && op.options.Int8(k, 0) != 0; };
    if (adj(oa, 0) || !adj(oa, 1) || adj(ob, 0) || adj(ob, 1)) continue;
    const int sc = oa.outputs[0], pr = os.outputs[0], ctx = ob.outputs[0];
    // what the SOFTMAX reads: the scores, or the ADD's output; exactly one ADD operand is the scores, the other
    // (the bias: a constant or a runtime tensor, int8) is only read and may have other readers
    int sm_in = sc, bias_t = -1, scores_operand = 0;
    if (E) {
      const TflOperator& oe = d.ops[E->op_index];
      if (oe.builtin != kTflAdd || oe.inputs.size() != 2 || oe.outputs.size() != 1) continue;
      if ((oe.inputs[0] == sc) == (oe.inputs[1] == sc)) continue;
      scores_operand = oe.inputs[0] == sc ? 0 : 1;
      bias_t = oe.inputs[1 - scores_operand];
      sm_in = oe.outputs[0];
      if (bias_t < 0 || E->out_tensor != sm_in || d.tensors[sm_in].type != DataType::kInt8 ||
          d.tensors[bias_t].type != DataType::kInt8 || !PrivateTensor(d, *sg, sm_in, S.op_index))
        continue;
    }
    if (os.inputs[0] != sm_in || ob.inputs[0] != pr || ob.inputs[1] == pr || A.out_tensor != sc || S.out_tensor != pr ||
        B.out_tensor != ctx)
      continue;
    if (d.tensors[sc].type != DataType::kInt8 || d.tensors[pr].type != DataType::kInt8) continue;
    if (!PrivateTensor(d, *sg, sc, E ? E->op_index : S.op_index) || !PrivateTensor(d, *sg, pr, B.op_index)) continue;
    const bh_batch_matmul_params &a = A.as<bh_batch_matmul_params>(), &b = B.as<bh_batch_matmul_params>();
    const bh_softmax_params& s = S.as<bh_softmax_params>();
    const bh_eltwise_params* ep = E ? &E->as<bh_eltwise_params>() : nullptr;
    if (ep) {
      // the scores operand has the output's shape [b0, b1, rows, keys]; the bias broadcasts to it
      const int so[4] = {a.batch[0], a.batch[1], a.m, a.n};
      const int* ss = scores_operand == 0 ? ep->shape_a : ep->shape_b;
      const int* sb = scores_operand == 0 ? ep->shape_b : ep->shape_a;
      bool ok = ep->kind == BH_ELT_ADD && ep->in_signed && (scores_operand == 0 ? ep->a : ep->b) == a.out;
      for (int k = 0; k < 4; ++k) ok = ok && ep->shape_o[k] == so[k] && ss[k] == so[k] && (sb[k] == 1 || sb[k] == so[k]);
      if (!ok) continue;
    }
    if (s.input != (ep ? ep->out : a.out) || s.output != b.lhs || !s.is_signed || s.depth != a.n ||
        s.rows != static_cast<long>(a.batch[0]) * a.batch[1] * a.m)
      continue;
    if (b.batch[0] != a.batch[0] || b.batch[1] != a.batch[1] || b.m != a.m || b.k != a.n) continue;
    Launch F;
    F.op_index = A.op_index;
    F.out_tensor = ctx;
    bh_attention_params& p = F.Set<Launch::kAttention>();
    p.batch[0] = a.batch[0];
    p.batch[1] = a.batch[1];
    p.rows = a.m;
    p.keys = a.n;
    p.head_dim = a.k;
    p.out_dim = b.n;
    p.q_inner_stride = p.k_inner_stride = p.v_inner_stride = p.out_inner_stride = 1;
    for (int k = 0; k < 2; ++k) {
      p.q_bstride[k] = a.lhs_bstride[k];
      p.k_bstride[k] = a.rhs_bstride[k];
      p.v_bstride[k] = b.rhs_bstride[k];
    }
    p.q_row_stride = a.lhs_row_stride;
    p.k_row_stride = a.rhs_col_stride;
    p.v_row_stride = b.rhs_k_stride;
    p.out_bstride[1] = static_cast<int64_t>(b.m) * b.n;
    p.out_bstride[0] = p.out_bstride[1] * b.batch[1];
    p.out_row_stride = b.n;
    p.qk = bh_attention_quant{a.lhs_zp, a.rhs_zp, a.out_zp, a.mult, a.shift, a.requant_fast};
    p.pv = bh_attention_quant{b.lhs_zp, b.rhs_zp, b.out_zp, b.mult, b.shift, b.requant_fast};
    p.table = s.table;
    p.sm_out_scale = s.out_scale;
    p.sm_out_zp = s.out_zp;
    p.q = a.lhs;
    p.k = a.rhs;
    p.v = b.rhs;
    p.out = b.out;
    if (ep) {
      const int* sb = scores_operand == 0 ? ep->shape_b : ep->shape_a;
      const int64_t st[4] = {static_cast<int64_t>(sb[1]) * sb[2] * sb[3], static_cast<int64_t>(sb[2]) * sb[3], sb[3], 1};
      p.bias = scores_operand == 0 ? ep->b : ep->a;
      p.bias_bstride[0] = sb[0] == 1 ? 0 : st[0];
      p.bias_bstride[1] = sb[1] == 1 ? 0 : st[1];
      p.bias_row_stride = sb[2] == 1 ? 0 : st[2];
      p.bias_key_stride = sb[3] == 1 ? 0 : st[3];
      p.add = bh_attention_add{ep->a_off,  ep->b_off,   ep->o_off,  ep->left_shift, ep->a_mult,  ep->a_shift,
                               ep->b_mult, ep->b_shift, ep->o_mult, ep->o_shift,    ep->act_min, ep->act_max};
      p.add_scores_operand = scores_operand;
    }
    // the head TRANSPOSEs around the pattern
    const int jq = absorb_in(i, oa.inputs[0], A.op_index, a.lhs, p.q_bstride, &p.q_row_stride, &p.q);
    const int jk = oa.inputs[1] == oa.inputs[0] ? -1
                                                : absorb_in(i, oa.inputs[1], A.op_index, a.rhs, p.k_bstride, &p.k_row_stride, &p.k);
    const int jv = ob.inputs[1] == oa.inputs[0] || ob.inputs[1] == oa.inputs[1]
                       ? -1
                       : absorb_in(i, ob.inputs[1], B.op_index, b.rhs, p.v_bstride, &p.v_row_stride, &p.v);
    int jo = -1;
    for (size_t j = i + 3 + e; j < ls.size() && jo < 0; ++j) {
      const Launch& r = ls[j];
      if (r.kind() != Launch::kReindex || r.as<bh_reindex_params>().input != b.out) continue;
      const TflOperator& op = d.ops[r.op_index];
      std::vector<int64_t> perm;
      if (!head_perm(op, &perm) || op.inputs[0] != ctx || r.out_tensor != op.outputs[0] ||
          !PrivateTensor(d, *sg, ctx, r.op_index))
        break;
      // ctx axis perm[k] is the TRANSPOSE's output axis k
      const std::vector<int64_t> ys = dense_strides(d.tensors[op.outputs[0]].shape);
      std::vector<int64_t> dm(perm.size()), st(perm.size());
      for (size_t k = 0; k < perm.size(); ++k) {
        dm[perm[k]] = d.tensors[ctx].shape[perm[k]];
        st[perm[k]] = ys[k];
      }
      operand(dm, st, p.out_bstride, &p.out_row_stride);
      p.out = r.as<bh_reindex_params>().output;
      F.out_tensor = r.out_tensor;
      jo = static_cast<int>(j);
    }
    if (bh_attention_i8_check(&p) != 0) continue;  // over a limit: the three (four) launches stay
    F.kernel = bh_attention_i8_kernel(&p);
    F.alg_ops = A.alg_ops + B.alg_ops;
    F.alg_bytes = static_cast<double>(meta_[oa.inputs[0]]->bytes + meta_[oa.inputs[1]]->bytes + meta_[ob.inputs[1]]->bytes +
                                      meta_[ctx]->bytes) + 1024.0;
    if (E) {
      F.alg_bytes += static_cast<double>(d.tensors[bias_t].num_elements());
      sg->fused_ops.insert(E->op_index);
      sg->fused_tensors.insert(sm_in);
    }
    sg->fused_ops.insert(S.op_index);
    sg->fused_ops.insert(B.op_index);
    sg->fused_tensors.insert(sc);
    sg->fused_tensors.insert(pr);
    for (int j : {jq, jk, jv}) {
      if (j < 0) continue;
      dead[j] = true;
      sg->fused_ops.insert(ls[j].op_index);
      sg->fused_tensors.insert(ls[j].out_tensor);
    }
    if (jo >= 0) {
      dead[jo] = true;
      sg->fused_ops.insert(ls[jo].op_index);
      sg->fused_tensors.insert(ctx);
    }
    for (size_t j = i + 1; j <= i + 2 + e; ++j) dead[j] = true;
    ls[i] = F;
    i += 2 + e;
  }
  DropDead(&ls, dead);
}

}  // namespace hip
}  // namespace band
