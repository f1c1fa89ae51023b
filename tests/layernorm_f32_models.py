"""Fixtures of the float32 LayerNorm as one launch (layernorm_f32_kernel,
BAND_HIP_FUSED_LAYERNORM_F32=1): the numpy restatement of the rule, its
deliberately wrong variants, the float64 LayerNorm with a derived error bound,
the launcher cases and data kinds, and the models.

The rule (include/band_hip_kernels.h holds it).  On a row x[0..C), every
operation one IEEE float32 operation - an explicit .astype(np.float32) after
each:

    m = S(x) / C                      d_i = (x_i - m)^2  (two roundings)
    v = S(d) / C      e = v + eps     r = 1 / sqrt(e)    (sqrt, then divide)
    g_i = r * gamma_i   a_i = x_i * g_i   b_i = m * g_i   c_i = beta_i - b_i   y_i = a_i + c_i

The sums S: lane l of 64 owns elements 256 j + 4 l + k (j, k = 0 .. 3; those
below C), starts from +0 and adds its own in ascending index order; the 64
lane sums meet in an xor butterfly over offsets 32, 16, 8, 4, 2, 1
(value[l] + value[l ^ o] in every lane).

The error bound of np_layernorm_f32 against layernorm_real, in
tests/float_harness.py's notation (u = 2^-24, gamma(n) = n u / (1 - n u)).
Hats are computed values.

  The sums.  C terms in any order and the division are C roundings on any
    path; in the rule's order a term passes through at most 15 additions in its
    lane (the first one, to +0, is exact), 6 in the butterfly and the division.
    N = min(C, 22):
        |m^ - m| <= dm = gamma(N) mean|x|.
  The variance.  t_i' = x_i - m^ has sum_i t_i'^2 / C = v + (m^ - m)^2 exactly
    (sum_i (x_i - m) = 0 removes the cross term).  d_i^ = t_i'^2 (1 + d1)^2 (1 + d2),
    then the sum of N more roundings over non-negative terms:
        |v^ - v| <= dv = dm^2 + gamma(N + 3) (v + dm^2).
  e^ = (v^ + eps)(1 + d):  |e^ - e| / e <= re = dv (1 + u) / e + u.
  r^ = fl(1 / fl(sqrt(e^))): sqrt(e / e^) = (1 + t)^(-1/2) with |t| <= re < 1, and
    |(1 + t)^(-1/2) - 1| <= h = (re / 2) (1 - re)^(-3/2) (mean value theorem: half
    of e's error to first order); the sqrt and the divide add one rounding each:
        |r^ - r| / r <= rr = (1 + h)(1 + gamma(2)) - 1.      (re >= 1: no bound, inf)
  g_i^ = r^ gamma_i (1 + d):  |g_i^ - g_i| / |g_i| <= rg = (1 + rr)(1 + u) - 1.
  The result is formed as x g - m g + beta, not as (x - m) g + beta:
        y_i^ = [x_i g_i^ (1 + da) + (beta_i - m^ g_i^ (1 + db))(1 + dc)](1 + dy)
    Without da .. dy that is y_i + (g_i^ - g_i)(x_i - m) - g_i^ (m^ - m); the product
    x g carries two roundings (da, dy), m g three, beta two:
        |y_i^ - y_i| <= |g_i| [ rg |x_i - m| + (1 + rg)(dm + gamma(3)(|x_i| + |m| + dm)) ]
                        + gamma(2) |beta_i| + 2^-126.
    The cancellation of x g against m g makes the bound absolute: it grows with
    |g_i| (|x_i| + |m|) and with the error of m, not with |y_i|.

tests/test_layernorm_f32_cpu.py judges the restatement against this bound and
against its wrong variants; tests/test_layernorm_f32_gpu.py holds the kernel to
the restatement bit for bit."""
import ctypes

import numpy as np

from band_amd.tflite_synth import OPC, FGraph, _encoder
from tests import float_harness as H
from tests import hybrid_models as Y

F = np.float32
F64 = np.float64
KERNEL = "layernorm_f32_kernel"
OP_KERNELS = ("mean_kernel", "eltwise_f32_kernel", "unary_f32_kernel")
FLAG = "BAND_HIP_FUSED_LAYERNORM_F32"
MAX_DEPTH = 1024
EPS = F(1e-6)
SLACK, NAN_WORD = Y.SLACK, Y.NAN_WORD
_LANES = np.arange(64)


# ---- the rule ----------------------------------------------------------------------------
def rule_sum(v, serial=False):
    """S over the last axis of float32 v [rows][C] in the rule's order (serial: index order, the wrong variant)"""
    v = np.asarray(v, F)
    rows, c = v.shape
    assert c <= MAX_DEPTH
    with np.errstate(invalid="ignore", over="ignore"):
        if serial:
            acc = np.zeros(rows, F)
            for i in range(c):
                acc = (acc + v[:, i]).astype(F)
            return acc
        pad = np.zeros((rows, MAX_DEPTH), F)
        pad[:, :c] = v
        own = pad.reshape(rows, 4, 64, 4)  # [step j][lane l][k]
        acc = np.zeros((rows, 64), F)
        for j in range(4):
            for k in range(4):
                acc = (acc + own[:, j, :, k]).astype(F)
        for o in (32, 16, 8, 4, 2, 1):
            acc = (acc + acc[:, _LANES ^ o]).astype(F)
    assert (acc.view(np.uint32) == acc[:, :1].view(np.uint32)).all() or np.isnan(acc).any()
    return acc[:, 0].copy()


def np_layernorm_f32(x, gamma, beta, eps, wrong=None):
    """float32 y [rows][C] of float32 rows x by the rule.  wrong: "serial" (sums in index order), "one_pass"
    (E[x^2] - m^2), "no_eps", "c_minus_1" (the variance divided by C - 1), "fma" (x g + c as one fused operation)"""
    x = np.asarray(x, F)
    gamma, beta, eps = np.asarray(gamma, F), np.asarray(beta, F), F(eps)
    rows, c = x.shape
    fc = F(c)
    serial = wrong == "serial"
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = (rule_sum(x, serial) / fc).astype(F)
        if wrong == "one_pass":
            sq = (x * x).astype(F)
            v = ((rule_sum(sq) / fc).astype(F) - (m * m).astype(F)).astype(F)
        else:
            t = (x - m[:, None]).astype(F)
            d = (t * t).astype(F)
            v = (rule_sum(d, serial) / (F(c - 1) if wrong == "c_minus_1" else fc)).astype(F)
        e = v if wrong == "no_eps" else (v + eps).astype(F)
        r = (F(1.0) / np.sqrt(e).astype(F)).astype(F)
        g = (r[:, None] * gamma[None, :]).astype(F)
        a = (x * g).astype(F)
        b = (m[:, None] * g).astype(F)
        cc = (beta[None, :] - b).astype(F)
        if wrong == "fma":
            return (x.astype(F64) * g.astype(F64) + cc.astype(F64)).astype(F)
        return (a + cc).astype(F)


def layernorm_real(x, gamma, beta, eps):
    """the LayerNorm of the float32 inputs in float64"""
    x = np.asarray(x, F).astype(F64)
    m = x.mean(axis=1, keepdims=True)
    v = ((x - m) ** 2).mean(axis=1, keepdims=True)
    return (x - m) / np.sqrt(v + float(F(eps))) * np.asarray(gamma, F).astype(F64) + np.asarray(beta, F).astype(F64)


def layernorm_bound(x, gamma, beta, eps):
    """the per-element bound derived in the module docstring"""
    x = np.asarray(x, F).astype(F64)
    gamma, beta = np.asarray(gamma, F).astype(F64), np.asarray(beta, F).astype(F64)
    c = x.shape[1]
    n = min(c, 22)
    u = H.U
    m = x.mean(axis=1, keepdims=True)
    v = ((x - m) ** 2).mean(axis=1, keepdims=True)
    e = v + float(F(eps))
    dm = H.gamma(n) * np.abs(x).mean(axis=1, keepdims=True)
    dv = dm ** 2 + H.gamma(n + 3) * (v + dm ** 2)
    re = dv * (1 + u) / e + u
    with np.errstate(invalid="ignore", divide="ignore"):
        h = np.where(re < 1, 0.5 * re * np.abs(1 - re) ** -1.5, np.inf)
    rr = (1 + h) * (1 + H.gamma(2)) - 1
    rg = (1 + rr) * (1 + u) - 1
    g = np.abs(gamma)[None, :] / np.sqrt(e)
    return g * (rg * np.abs(x - m) + (1 + rg) * (dm + H.gamma(3) * (np.abs(x) + np.abs(m) + dm))) + \
        H.gamma(2) * np.abs(beta)[None, :] + H.FLOOR


# ---- launcher cases ----------------------------------------------------------------------
# a partial workgroup, partial lanes, depths that are no multiple of 4, variance exactly 0 at depth 1, the limit
SHAPES = ((1, 1), (3, 5), (7, 64), (5, 65), (17, 48), (4, 192), (2, 1000), (9, 1023), (1, 1024))
KINDS = ("normal", "cancel", "const", "zeros")
NONFINITE_SHAPE = (5, 65)
MODES = ("out", "q_sym", "q_asym", "both_sym", "both_asym")
SEED = 2024  # chosen on the CPU so that "serial" and "fma" differ bit-wise from the rule (test_layernorm_f32_cpu.py)


class LnCase:
    def __init__(self, rows, depth, kind, seed=SEED):
        rng = np.random.default_rng(seed + 131 * rows + depth + 7 * len(kind))
        self.rows, self.depth, self.kind = rows, depth, kind
        self.gamma = rng.uniform(0.5, 1.5, depth).astype(F)
        self.beta = rng.normal(0.0, 0.3, depth).astype(F)
        self.eps = EPS
        if kind == "normal":
            x = rng.normal(0, 1, (rows, depth))
        elif kind == "cancel":
            x = 1000.0 + rng.normal(0, 1e-2, (rows, depth))
        elif kind == "const":
            x = np.repeat(rng.normal(0, 1, (rows, 1)), depth, axis=1)
        elif kind == "zeros":
            x = np.zeros((rows, depth))
        else:
            assert kind == "nonfinite" and rows >= 5 and depth >= 8
            x = rng.normal(0, 1, (rows, depth))
            x[1, 3] = np.inf    # row 1: m = inf, x - m has inf - inf at [1, 3]: the whole row NaN
            x[2, 0] = -np.inf
            x[2, depth - 1] = np.inf  # row 2: inf - inf in the sum: the whole row NaN
            x[3, 7] = np.nan    # row 3: NaN; rows 0 and 4 stay finite
        self.x = x.astype(F)
        self.name = "%dx%d_%s" % (rows, depth, kind)

    def ref(self, wrong=None):
        return np_layernorm_f32(self.x, self.gamma, self.beta, self.eps, wrong)

    def real(self):
        return layernorm_real(self.x, self.gamma, self.beta, self.eps)

    def bound(self):
        return layernorm_bound(self.x, self.gamma, self.beta, self.eps)


def launcher_cases():
    return [LnCase(r, d, k) for r, d in SHAPES for k in KINDS]


def params(rows, depth, eps=EPS):
    from band_amd import _abi
    p = _abi.LayerNormF32Params()
    p.rows, p.depth, p.eps = rows, depth, float(eps)
    return p


def launch(case, lib, mode, off=0, rows=None):
    """The case (its first `rows` rows) through bh_layernorm_f32 on the device.  mode: one of MODES.  off = 4: the
    input, gamma, beta and the output 4 bytes off their 16-byte aligned buffers and q 1 byte off its.  Every
    output lies in a buffer filled with a pattern whose SLACK trailing bytes, the bytes in front of a moved
    pointer and - for an output the mode leaves unset - every byte must stay.
    Returns (y, q, s, offset), None for what the mode does not write."""
    from band_amd import _abi
    r, d = (case.rows if rows is None else rows), case.depth
    want_y, want_q = mode == "out" or mode.startswith("both"), mode != "out"
    q_off = 1 if off else 0

    def in_buf(a):
        return Y.buffer(np.concatenate([np.zeros(off, np.uint8), np.ascontiguousarray(a).view(np.uint8).reshape(-1)]),
                        True)

    def out_buf(nbytes, o, word):
        return Y.buffer(Y._filled(o + nbytes + SLACK, word), True)

    dx, dg, db = in_buf(case.x[:r]), in_buf(case.gamma), in_buf(case.beta)
    dy = out_buf(4 * r * d, off, NAN_WORD)
    dq = out_buf(r * d, q_off, 0xa5a5a5a5)
    ds, do = out_buf(4 * r, 0, NAN_WORD), out_buf(4 * r, 0, 0xa5a5a5a5)
    p = params(r, d, case.eps)
    p.input, p.gamma, p.beta = dx.value + off, dg.value + off, db.value + off
    p.output = dy.value + off if want_y else None
    if want_q:
        p.q, p.scale, p.offset = dq.value + q_off, ds.value, do.value
    p.asymmetric = int(mode.endswith("asym"))
    assert lib.bh_layernorm_f32_kernel(ctypes.byref(p)) == KERNEL.encode(), lib.bh_last_error()
    _abi.check(lib.bh_layernorm_f32(ctypes.byref(p), None), "bh_layernorm_f32")

    def take(buf, nbytes, o, word, dtype, shape, written):
        got = buf.download(np.uint8, (o + nbytes + SLACK,))
        fill = Y._filled(o + nbytes + SLACK, word)
        if not written:
            assert (got == fill).all(), "%s %s: an output the mode leaves unset was written" % (case.name, mode)
            return None
        assert (got[:o] == fill[:o]).all(), "%s %s: bytes in front of the output were written" % (case.name, mode)
        assert (got[o + nbytes:] == fill[o + nbytes:]).all(), "%s %s: bytes past the output were written" % (case.name, mode)
        return got[o:o + nbytes].copy().view(dtype).reshape(shape)

    y = take(dy, 4 * r * d, off, NAN_WORD, F, (r, d), want_y)
    q = take(dq, r * d, q_off, 0xa5a5a5a5, np.int8, (r, d), want_q)
    s = take(ds, 4 * r, 0, NAN_WORD, F, (r,), want_q)
    o = take(do, 4 * r, 0, 0xa5a5a5a5, np.int32, (r,), want_q)
    return y, q, s, o


def valid_block(ptr):
    """a LayerNormF32Params the check accepts, every pointer `ptr` (16-byte aligned)"""
    p = params(3, 40)
    p.input = p.gamma = p.beta = p.output = p.q = p.scale = p.offset = ptr
    return p


# (name, the change, the reason bh_last_error names)
REFUSALS = [("null_input", dict(input=None), "null input, gamma or beta"),
            ("null_gamma", dict(gamma=None), "null input, gamma or beta"),
            ("null_beta", dict(beta=None), "null input, gamma or beta"),
            ("no_output", dict(output=None, q=None, scale=None, offset=None), "neither output nor q"),
            ("q_without_scale", dict(scale=None), "all set or all null"),
            ("q_without_offset", dict(offset=None), "all set or all null"),
            ("scale_without_q", dict(q=None), "all set or all null"),
            ("zero_rows", dict(rows=0), "non-positive rows or depth"),
            ("zero_depth", dict(depth=0), "non-positive rows or depth"),
            ("negative_depth", dict(depth=-3), "non-positive rows or depth"),
            ("depth_above_limit", dict(depth=MAX_DEPTH + 1), "depth above 1024"),
            ("rows_2_31", dict(rows=1 << 31), "2^31 or more rows")]


# ---- models ------------------------------------------------------------------------------
def ln_only():
    """LayerNorm of a 5 x 48 input; y is the output"""
    g = FGraph(seed=81, name="ln_only", hybrid="symmetric")
    g.output(g.layer_norm(g.input([5, 48])))
    return g.build()


LN_OP_OF = {"m": 0, "a": 6}  # which of the ten ops makes the row mean m, the per-element a = x * g


def ln_with_intermediate_output(which):
    """LayerNorm alone on [1, 3, 5] (three rows, depth 5: below every vector width of the kernels) whose
    outputs are y and one intermediate of the pattern, `which` of LN_OP_OF"""
    g = FGraph(seed=85, name="ln_out_" + which, hybrid="symmetric")
    g.output(g.layer_norm(g.input([1, 3, 5])))
    g.output(g.mb.ops[-10:][LN_OP_OF[which]]["outputs"][0])
    return g.build()


QKV_UNITS = (20, 16, 33)


def ln_qkv(form):
    """LayerNorm, then three hybrid FULLY_CONNECTEDs of one form whose outputs are the model's"""
    g = FGraph(seed=82, name="ln_qkv_" + form, hybrid=form)
    y = g.layer_norm(g.input([1, 7, 48]))
    for units in QKV_UNITS:
        g.output(g.fully_connected(y, units, keep_num_dims=True))
    return g.build()


def ln_fc_and_add():
    """one hybrid FULLY_CONNECTED on y, and ADD(y, x) reading y as well"""
    g = FGraph(seed=83, name="ln_fc_and_add", hybrid="asymmetric")
    x = g.input([1, 7, 48])
    y = g.layer_norm(x)
    g.output(g.fully_connected(y, 20, keep_num_dims=True))
    g.output(g.add(y, x))
    return g.build()


def ln_mixed():
    """one symmetric and one asymmetric hybrid FULLY_CONNECTED on the same y (the symmetric one reads first)"""
    g = FGraph(seed=84, name="ln_mixed", hybrid="symmetric")
    y = g.layer_norm(g.input([1, 7, 48]))
    g.output(g.fully_connected(y, 20, keep_num_dims=True, hybrid="symmetric"))
    g.output(g.fully_connected(y, 16, keep_num_dims=True, hybrid="asymmetric"))
    return g.build()


def encoder_with_qkv_outputs(form, shape=(17, 48, 3, 96)):
    """hybrid_models' encoder block of `shape` with the first attention's Q, K and V projections as extra outputs"""
    t, c, heads, hidden = shape
    g = FGraph(8, "encoder_block_f32_hybrid_qkv", hybrid=form)
    g.output(_encoder(g, g.input([1, t, c]), heads, hidden))
    fcs = [o for o in g.mb.ops if g.mb.opcodes[o["opcode"]][0] == OPC["FULLY_CONNECTED"]]
    for o in fcs[:3]:
        g.output(o["outputs"][0])
    return g.build()


MODELS = {"ln_only": ln_only, "ln_qkv_symmetric": lambda: ln_qkv("symmetric"),
          "ln_qkv_asymmetric": lambda: ln_qkv("asymmetric"), "ln_fc_and_add": ln_fc_and_add, "ln_mixed": ln_mixed}
ENCODERS = ("encoder_17_48_3_96_symmetric", "encoder_17_48_3_96_asymmetric")


def layer_norms(om):
    """[(x, gamma, beta, eps, y)] tensor indices of the LayerNorm patterns of an oracle model, in op order"""
    out = []
    ops = om.operators
    for i, o in enumerate(ops):
        if o.builtin == Y.MEAN and i + 9 < len(ops) and ops[i + 2].builtin == Y.MEAN and \
                ops[i + 1].inputs[0] == o.inputs[0]:
            out.append((o.inputs[0], ops[i + 5].inputs[1], ops[i + 8].inputs[0], ops[i + 3].inputs[1],
                        ops[i + 9].outputs[0]))
    return out


def model_layernorm(om, ln, x):
    """np_layernorm_f32 of pattern `ln` of layer_norms(om) on input x, as rows"""
    tx, tg, tb, te, ty = ln
    T = om.tensors
    depth = T[tx].shape[-1]
    return np_layernorm_f32(np.asarray(x, F).reshape(-1, depth), T[tg].data, T[tb].data, F(T[te].data.reshape(-1)[0]))


def fc_from_rows(om, o, y_rows):
    """the hybrid FULLY_CONNECTED o of the model on the float32 rows y_rows, by the rule, in the op's output shape"""
    T = om.tensors
    w = T[o.inputs[1]]
    bias = T[o.inputs[2]].data if len(o.inputs) > 2 and o.inputs[2] >= 0 else None
    opt = o.options
    act = Y.ACTS[opt.scalar(0, "b", 0)] if opt is not None else "NONE"
    asym = bool(opt.scalar(3, "b", 0)) if opt is not None else False
    q, s, off = Y.np_dynquant(y_rows, asym)
    return Y.np_fc_from_q(q, s, off, w.data, float(w.scale[0]), bias, act).reshape(T[o.outputs[0]].shape)
