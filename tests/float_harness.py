"""Float32 parity harness: float64 references of the float ops and per-element
error bounds derived from the arithmetic (not tuned), shared by the kernel
tests (tests/test_float_kernels_gpu.py), the per-op residual checks of the
executor (tests/test_float_ops_cpu.py) and the self-check of the bounds
(tests/test_float_harness_cpu.py).

Notation: u = 2^-24 is the unit roundoff of float32, gamma(n) = n u / (1 - n u)
bounds the relative error of a product of n factors (1 + d_i), |d_i| <= u
(Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1).  The
references are evaluated in float64 (unit roundoff 2^-53; their own error is
below 2^-29 of every bound here) and are NOT rounded to float32.

CONV_2D / DEPTHWISE_CONV_2D / FULLY_CONNECTED
    y = sum_k x_k w_k + bias, any summation order, with or without FMA.
    Every term passes through at most K - 1 additions and one product
    rounding, then the bias add and (for split-K) up to 16 partial sums that
    meet in a further 15 additions: at most K + 18 roundings on any path, so
        |got - y| <= gamma(K + 18) (sum_k |x_k| |w_k| + |bias|) + 2^-126.
    K = k_h k_w in_c (k_h k_w for depthwise, depth for FC).  The magnitude sum
    is the same reference evaluated on |x|, |w|, |bias| (clipped taps drop out
    of both).  The fused activation min(max(v, lo), hi) is 1-Lipschitz, so the
    bound holds after it.  2^-126 lets a denormal result flush to zero.

AVERAGE_POOL_2D
    count - 1 additions and one division (the count converts exactly):
        |got - y| <= gamma(count + 1) mean |x|,  count = the clipped window.
MAX_POOL_2D, RELU / RELU6 / RELU_N1_TO_1: selections, exact.

ADD / SUB / MUL: one rounding, |got - y| <= u |y|.
SQUARED_DIFFERENCE: fl(fl(a - b)^2) = (a - b)^2 (1 + d1)^2 (1 + d2):
    |got - y| <= gamma(3) |y|.
    (|y| is taken before the activation clamp; the clamp is 1-Lipschitz.)

LOGISTIC  y = 1 / (1 + e), e = exp(-x)
    The HIP math API reference (ROCm documentation, "HIP math API", table of
    single-precision functions) lists expf with a maximum error of 1 ulp;
    the CPU worker's glibc expf is below 1 ulp.  EXPF_ULP = 1 ulp is at most
    2 u relative (an ulp of v is at most 2^-23 |v|).  With e' = e (1 + 2 t u),
    |t| <= EXPF_ULP, the sum 1 + e' moves by the relative amount
    2 t u e / (1 + e) < 2 EXPF_ULP u; the add and the (correctly rounded,
    HIP's default for float division) divide contribute one u each:
        |got - y| <= gamma(2 EXPF_ULP + 2) |y| + 2^-126 = gamma(4) |y| + 2^-126.
    The floor covers e' = +inf (y' = 0 where y is denormal).
RSQRT  y = 1 / sqrt(x): one correctly rounded sqrt, one correctly rounded
    divide: |got - y| <= gamma(2) |y| + 2^-126.  No expf involved.

SOFTMAX  y_k = e_k / S, e_k = exp(a_k), a_k = (x_k - max) beta, S = sum_j e_j
    * argument: fl(fl(x_k - max) beta) has |a_k' - a_k| <= 2 u |a_k|
      <= 2 u beta (max - min); exp turns an absolute argument error into the
      same relative error of e_k:              2 beta (max - min) u
    * expf in the numerator, EXPF_ULP = 1 ulp:                       2 u
    * S: every summand carries its own expf error (a weighted mean of
      errors of at most 2 u:                                         2 u)
      and the sum of depth positive terms adds at most (depth - 1) u in
      any order.  The argument errors of the summands enter S weighted by
      e_j / S, i.e. by terms |a_j| e^{a_j} <= 1 / e against S >= 1; they are
      carried by the depth term, of which a wave-strided sum with a butterfly
      (depth / 64 + 6 additions per path) uses only a small part.
                                                        (depth - 1) u + 2 u
    * the reciprocal 1 / S and the product, one rounding each:       2 u
    * second-order terms:                                          <  1 u
        |got - y| <= (2 beta (max - min) + depth + 8) u |y| + 2^-126.
    Where exp((x_k - max) beta) underflows the reference is below 2^-126 and
    0 is accepted by the floor.

MEAN over the last axis of n values: n - 1 additions in any order and one
    division, n roundings, each relative to a partial sum of at most sum|x|:
        |got - y| <= gamma(n) mean |x| + 2^-126.
GELU: tests.encoder_models.gelu_f32_bound, which takes the ulp count of the
    library's erf / tanh (1 for glibc, 16 for the device library).
BATCH_MATMUL: |got - y| <= gamma(K + 2) sum_k |a_k| |b_k| + 2^-126.
TRANSPOSE, the slicing ops, SPLIT / SPLIT_V, DEPTH_TO_SPACE / SPACE_TO_DEPTH
    copy elements: exact (tests.reindex_models.eval_reindex).

Non-finite values: the comparison first requires NaN exactly where the
reference has NaN and +-inf exactly where it has +-inf; numpy's clip
propagates NaN as TFLite's std::min(std::max(v, lo), hi) does.
"""
import numpy as np

from oracle import float_ref as F
from tests import encoder_models as E
from tests import reindex_models as R

U = 2.0 ** -24
FLOOR = 2.0 ** -126
EXPF_ULP = 1  # HIP math API reference: expf, maximum error 1 ulp
INF = float("inf")
F64 = np.float64

ACT = {"NONE": (-INF, INF), "RELU": (0.0, INF), "RELU_N1_TO_1": (-1.0, 1.0), "RELU6": (0.0, 6.0)}
ACT_BY_CODE = {0: ACT["NONE"], 1: ACT["RELU"], 2: ACT["RELU_N1_TO_1"], 3: ACT["RELU6"]}


def gamma(n):
    n = np.asarray(n, F64)
    return n * U / (1.0 - n * U)


# ---- geometry (kernels/padding.h: ComputeOutSize / ComputePadding) ---------
def out_size(same, n, k, stride, dilation=1):
    eff = (k - 1) * dilation + 1
    return (n + stride - 1) // stride if same else (n + stride - eff) // stride


def padding(stride, dilation, n, k, out):
    eff = (k - 1) * dilation + 1
    return max(0, (out - 1) * stride + eff - n) // 2


class Geom:
    """window geometry of a conv / pool over an [h, w] map"""

    def __init__(self, in_hw, k_hw, stride=1, dilation=1, same=True):
        pair = lambda v: (v, v) if np.isscalar(v) else tuple(v)  # noqa: E731
        self.in_hw, self.k_hw = tuple(in_hw), tuple(k_hw)
        self.stride, self.dilation = pair(stride), pair(dilation)
        self.out_hw = tuple(out_size(same, self.in_hw[i], self.k_hw[i], self.stride[i], self.dilation[i])
                            for i in range(2))
        self.pad = tuple(padding(self.stride[i], self.dilation[i], self.in_hw[i], self.k_hw[i], self.out_hw[i])
                         for i in range(2))


# ---- references: (float64 result, per-element bound or None for exact) -----
def conv_ref(x, w, bias, g, act=(-INF, INF), depth_multiplier=None):
    """x [N,H,W,C]; w OHWI, or [1,KH,KW,C*dm] with depth_multiplier set"""
    def run(x_, w_, b_, lo, hi):
        if depth_multiplier:
            return F.dwconv2d_f32(x_, w_, b_, depth_multiplier, g.stride, g.dilation, g.pad, g.out_hw, lo, hi,
                                  out_dtype=F64)
        return F.conv2d_f32(x_, w_, b_, g.stride, g.dilation, g.pad, g.out_hw, lo, hi, out_dtype=F64)
    ref = run(x, w, bias, *act)
    mag = run(np.abs(x), np.abs(w), None if bias is None else np.abs(bias), -INF, INF)
    k = w.shape[1] * w.shape[2] * (1 if depth_multiplier else w.shape[3])
    return ref, gamma(k + 18) * mag + FLOOR


def fc_ref(x, w, bias, act=(-INF, INF)):
    """x [..., depth] as rows, w [units, depth]"""
    ref = F.fully_connected_f32(x, w, bias, *act, out_dtype=F64)
    mag = F.fully_connected_f32(np.abs(x), np.abs(w), None if bias is None else np.abs(bias), -INF, INF,
                                out_dtype=F64)
    return ref, gamma(w.shape[1] + 18) * mag + FLOOR


def pool_ref(x, kind, g, act=(-INF, INF)):
    """kind "avg" / "max"; g.k_hw is the filter.  The maximum ignores NaN
    (std::max(acc, v) keeps acc when v is NaN, as fmaxf does) and starts at
    -inf, as both workers do."""
    n, ih, iw, c = x.shape
    (fh, fw), (sh, sw), (ph, pw), (oh, ow) = g.k_hw, g.stride, g.pad, g.out_hw
    xd = x.astype(F64)
    ref = np.zeros((n, oh, ow, c))
    mag = np.zeros((n, oh, ow, c))
    cnt = np.zeros((1, oh, ow, 1))
    with np.errstate(invalid="ignore"):
        for oy in range(oh):
            y0 = oy * sh - ph
            for ox in range(ow):
                x0 = ox * sw - pw
                win = xd[:, max(0, y0):min(ih, y0 + fh), max(0, x0):min(iw, x0 + fw)]
                win = win.reshape(n, -1, c)
                cnt[0, oy, ox, 0] = win.shape[1]
                if kind == "avg":
                    ref[:, oy, ox] = win.sum(axis=1) / win.shape[1]
                    mag[:, oy, ox] = np.abs(win).sum(axis=1) / win.shape[1]
                else:
                    ref[:, oy, ox] = np.fmax.reduce(win, axis=1, initial=-INF)
    ref = np.clip(ref, *act)
    return ref, (gamma(cnt + 1) * mag if kind == "avg" else None)


def eltwise_ref(a, b, kind, act=(-INF, INF)):
    """kind "add" / "sub" / "mul" / "sqdiff", numpy broadcasting"""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    with np.errstate(invalid="ignore"):
        v = a + b if kind == "add" else a - b if kind == "sub" else a * b if kind == "mul" else (a - b) * (a - b)
    rel = gamma(3) if kind == "sqdiff" else U
    return np.clip(v, *act), rel * np.abs(v)


def clamp_ref(x, lo, hi):
    return np.clip(np.asarray(x, F64), lo, hi), None


def logistic_ref(x):
    with np.errstate(over="ignore"):
        ref = F.logistic_f32(np.asarray(x), out_dtype=F64)
    return ref, gamma(2 * EXPF_ULP + 2) * np.abs(ref) + FLOOR


def rsqrt_ref(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = 1.0 / np.sqrt(np.asarray(x, F64))
    return ref, gamma(2) * np.abs(ref) + FLOOR


def softmax_ref(x, beta):
    x = np.asarray(x)
    depth = x.shape[-1]
    with np.errstate(invalid="ignore"):
        ref = F.softmax_f32(x, beta, out_dtype=F64)
        fin = np.where(np.isfinite(x), x.astype(F64), np.nan)
        all_nan = np.isnan(fin).all(axis=-1, keepdims=True)
        fin = np.where(all_nan, 0.0, fin)
        spread = np.nanmax(fin, axis=-1, keepdims=True) - np.nanmin(fin, axis=-1, keepdims=True)
        return ref, (2.0 * beta * spread + depth + 8) * U * np.abs(ref) + FLOOR


# ---- comparison ------------------------------------------------------------
def check(got, ref, tol, what=""):
    """Asserts |got - ref| <= tol element-wise (tol None: got == float32(ref)),
    NaN / +-inf exactly where ref has them; prints and returns the largest
    |got - ref| / tol over the finite elements."""
    got = np.asarray(got)
    ref = np.asarray(ref, F64)
    assert got.size == ref.size, "%s: %d elements, reference has %d" % (what, got.size, ref.size)
    if tol is None:
        ref = ref.astype(np.float32).astype(F64)
        tol = 0.0
    tol = np.broadcast_to(np.asarray(tol, F64), ref.shape).reshape(-1)
    got = got.astype(F64).reshape(-1)
    ref = ref.reshape(-1)
    nan, inf = np.isnan(ref), np.isinf(ref)
    fin = ~(nan | inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.where(fin, np.abs(got - ref), 0.0)
        bad = (nan != np.isnan(got)) | (inf & (got != ref)) | (fin & ~(err <= tol))
        ratio = np.where(err == 0, 0.0, err / np.where(fin, tol, 1.0))
    worst = float(ratio[fin].max()) if fin.any() else 0.0
    print("float-parity %s: max |got - ref| / tol = %.3g" % (what, worst))
    if bad.any():
        idx = np.flatnonzero(bad)
        lines = ["  [%d] got %r ref %r tol %.3g" % (i, got[i], ref[i], tol[i]) for i in idx[:8]]
        raise AssertionError("%s: %d of %d elements outside the bound (worst ratio %.3g)\n%s"
                             % (what, idx.size, ref.size, worst, "\n".join(lines)))
    return worst


def accepts(got, ref, tol):
    try:
        check(got, ref, tol, "self-check")
        return True
    except AssertionError:
        return False


# ---- graphs: one reference per op, on the executor's own inputs ------------
SQUARED_DIFFERENCE, RSQRT, BATCH_MATMUL, GELU = 99, 76, 126, 150  # BuiltinOperator codes the oracle's table leaves out


def _const(om, t):
    """float32 value of a constant tensor, or of the DEQUANTIZE of an fp16 constant"""
    tt = om.tensors[t]
    if tt.is_const:
        return tt.data.astype(np.float32)
    for o in om.operators:
        if o.outputs[0] == t and o.name == "DEQUANTIZE" and om.tensors[o.inputs[0]].is_const:
            return om.tensors[o.inputs[0]].data.astype(np.float32)
    return None


def op_reference(om, o, vals, gelu_ulps=1):
    """(float64 reference, bound or None) of operator o, its inputs taken from
    vals {tensor: array} where present and from the model's constants otherwise"""
    def get(i):
        t = o.inputs[i]
        if t < 0:
            return None
        if t in vals:
            return np.asarray(vals[t]).reshape(om.tensors[t].shape)
        return _const(om, t)
    opt, name, code = o.options, o.name, o.builtin
    act_of = lambda slot: ACT_BY_CODE[opt.scalar(slot, "b", 0) if opt is not None else 0]  # noqa: E731
    x = get(0)
    if name == "DEQUANTIZE":
        return x.astype(F64), None  # float16 -> float32 is exact
    if name in ("CONV_2D", "DEPTHWISE_CONV_2D"):
        dw = name == "DEPTHWISE_CONV_2D"
        w = get(1)
        bias = get(2) if len(o.inputs) > 2 else None
        sw, sh = opt.scalar(1, "i", 1), opt.scalar(2, "i", 1)
        dlw, dlh = (opt.scalar(5, "i", 1), opt.scalar(6, "i", 1)) if dw else (opt.scalar(4, "i", 1),
                                                                               opt.scalar(5, "i", 1))
        g = Geom(x.shape[1:3], w.shape[1:3], (sh, sw), (dlh, dlw), opt.scalar(0, "b", 0) == 0)
        return conv_ref(x, w, bias, g, act_of(4 if dw else 3), w.shape[3] // x.shape[3] if dw else None)
    if name == "FULLY_CONNECTED":
        return fc_ref(x, get(1), get(2) if len(o.inputs) > 2 else None, act_of(0))
    if name in ("ADD", "SUB", "MUL") or code == SQUARED_DIFFERENCE:
        kind = {"ADD": "add", "SUB": "sub", "MUL": "mul"}.get(name, "sqdiff")
        return eltwise_ref(x, get(1), kind, act_of(0) if code != SQUARED_DIFFERENCE else ACT["NONE"])
    if name in ("AVERAGE_POOL_2D", "MAX_POOL_2D"):
        g = Geom(x.shape[1:3], (opt.scalar(4, "i", 1), opt.scalar(3, "i", 1)),
                 (opt.scalar(2, "i", 1), opt.scalar(1, "i", 1)), 1, opt.scalar(0, "b", 0) == 0)
        return pool_ref(x, "avg" if name == "AVERAGE_POOL_2D" else "max", g, act_of(5))
    if name in ("RELU", "RELU6", "RELU_N1_TO_1"):
        return clamp_ref(x, *ACT[name])
    if name == "LOGISTIC":
        return logistic_ref(x)
    if code == RSQRT:
        return rsqrt_ref(x)
    if name == "SOFTMAX":
        return softmax_ref(x, opt.scalar(0, "f", 1.0) if opt is not None else 1.0)
    if name == "RESHAPE":
        return x.astype(F64), None
    if name == "MEAN":
        assert [int(v) for v in om.tensors[o.inputs[1]].data.reshape(-1)] in ([-1], [x.ndim - 1])
        keep = om.tensors[o.outputs[0]].shape
        ref = x.astype(F64).mean(axis=-1).reshape(keep)
        mag = np.abs(x).astype(F64).mean(axis=-1).reshape(keep)
        return ref, gamma(x.shape[-1]) * mag + FLOOR
    if code == GELU:
        approx = bool(opt.scalar(0, "b", 0)) if opt is not None else False
        ref = np.vectorize(lambda v: E.gelu_real(float(v), approx))(x).astype(F64)
        return ref, E.gelu_f32_bound(x, ref, gelu_ulps)
    if code == BATCH_MATMUL:
        adj_x = bool(opt.scalar(0, "b", 0)) if opt is not None else False
        adj_y = bool(opt.scalar(1, "b", 0)) if opt is not None else False
        a, b = x.astype(F64), get(1).astype(F64)
        a = np.swapaxes(a, -1, -2) if adj_x else a
        b = np.swapaxes(b, -1, -2) if adj_y else b
        return np.matmul(a, b), gamma(a.shape[-1] + 2) * np.matmul(np.abs(a), np.abs(b)) + FLOOR
    if code in R.REINDEX_OPS:
        return R.eval_reindex(om, o, vals)[0].astype(F64), None
    raise NotImplementedError("float harness: op %s" % name)


def graph_reference(om, feed):
    """every tensor of the graph, each op's float64 reference rounded to float32"""
    vals = {t: np.asarray(v, np.float32) for t, v in feed.items()}
    for o in om.operators:
        ref, _ = op_reference(om, o, vals)
        vals[o.outputs[0]] = ref.astype(np.float32).reshape(om.tensors[o.outputs[0]].shape)
    return vals


def check_graph_ops(om, vals, what="", gelu_ulps=1):
    """Each op against its reference on the tensors in vals (the executor's
    own).  A dynamic-range FULLY_CONNECTED / CONV_2D / DEPTHWISE_CONV_2D (int8
    weights) must equal its rule bit for bit (tests.hybrid_models,
    tests.hybrid_conv_models); every other op is held to op_reference's bound.
    gelu_ulps: 1 for glibc, 16 for the device library.  Returns ({op name:
    largest |got - ref| / tol}, {"fc", "conv": bit-exact ops checked})."""
    from tests import hybrid_conv_models as C
    from tests import hybrid_models as Y
    worst, exact = {}, {"fc": 0, "conv": 0}
    for i, o in enumerate(om.operators):
        got = vals[o.outputs[0]]
        rule = ("fc", Y.hybrid_fc_reference) if Y.is_hybrid_fc(om, o) else \
            ("conv", C.hybrid_conv_reference) if C.is_hybrid_conv(om, o) else None
        if rule:
            np.testing.assert_array_equal(np.asarray(got).reshape(om.tensors[o.outputs[0]].shape),
                                          rule[1](om, o, vals[o.inputs[0]]),
                                          err_msg="%s op %d hybrid %s" % (what, i, o.name))
            exact[rule[0]] += 1
            continue
        with np.errstate(invalid="ignore"):  # inf - inf in a non-finite case
            ref, tol = op_reference(om, o, vals, gelu_ulps)
        name = {SQUARED_DIFFERENCE: "SQUARED_DIFFERENCE", RSQRT: "RSQRT"}.get(o.builtin, o.name)
        r = check(got, ref, tol, "%s op %d %s" % (what, i, name))
        worst[name] = max(worst.get(name, 0.0), r)
    return worst, exact


def run_executor(buf, feeds, flag, worker, view_all):
    """Runs model bytes on one HipModelExecutor, once per feed of the list
    (on the GPU worker: eager, capture, graph replay); returns (oracle model,
    [{tensor: array}, ...]) of every op output (view_all) or of the graph
    outputs only."""
    from band_amd import HipModel, HipModelExecutor, SubgraphKey
    from oracle.tflite_fb import Model as OModel
    om = OModel(buf)
    m = HipModel(0)
    assert m.FromBuffer(buf).ok()
    ex = HipModelExecutor(0, worker, flag)
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st
    key = SubgraphKey(0, worker)
    want = sorted({t for o in om.operators for t in o.outputs}) if view_all else list(om.outputs)
    views = {t: ex.GetTensorView(key, t) for t in want}
    runs = []
    for feed in feeds:
        for t in om.inputs:
            ex.GetTensorView(key, t).GetData()[...] = feed[t]
        assert ex.ExecuteSubgraph(key).ok()
        vals = {t: v.GetData().copy() for t, v in views.items()}
        for t in om.inputs:
            vals[t] = np.asarray(feed[t], np.float32)
        runs.append(vals)
    return om, runs
