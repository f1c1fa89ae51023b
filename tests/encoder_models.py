"""Fixtures of the LayerNorm / GELU ops (int8 MEAN over the last axis,
SQUARED_DIFFERENCE, RSQRT, GELU): numpy restatements written from the formulas
(TFLite 2.9.2 reduce.cc, squared_difference.cc, elementwise.cc, activations.cc)
and not from the C++ of this project, the launcher cases, the models and
eval_encoder_op (one operator for tests.graph_reference).

Parity unpinned: no fixture of the reference holds outputs of these ops, and the
TFLite sources are not at hand; the restatements follow the arithmetic as it is
written in the docstrings below.  tests/test_layernorm_cpu.py holds each of them
against the real-valued function at a derived bound, so a misremembered constant
cannot pass unnoticed.

QuantizeMultiplier comes from the oracle's C code (oracle.runner), which the C++
does not share."""
import ctypes
import math

import numpy as np

from band_amd.tflite_synth import QGraph, encoder_block, vit_tiny
from oracle import runner as orc
from tests.fixed_point import mbqm, rdbypot, round_half_away, sat_shl, srdhm
from tests.grouped_models import SLACK, _buffer

MEAN, RSQRT, SQUARED_DIFFERENCE, GELU = 40, 76, 99, 150
MEAN_KERNEL, SQDIFF_KERNEL = "mean_rows_kernel", "eltwise_sqdiff_kernel"
F = np.float32


# ---- the four ops ---------------------------------------------------------------------
def np_mean_rows(x, s_in, z_in, s_out, z_out):
    """MEAN over the last axis of an int8 / uint8 array.  Equal quantisation:
    out = (T)(sum / n), C++ integer division.  Otherwise, in float32, one
    operation at a time: scale = s_in / s_out; bias = -z_in * scale + 0.5f;
    mean = (float)sum / (float)n; r = round(mean * scale + bias) + z_out; clamp."""
    n = x.shape[-1]
    s = x.astype(np.int64).sum(-1)
    info = np.iinfo(x.dtype)
    if F(s_in) == F(s_out) and z_in == z_out:
        q = np.abs(s) // n * np.sign(s)
        return q.astype(x.dtype)
    scale = F(s_in) / F(s_out)
    bias = F(-z_in) * scale + F(0.5)
    mean = s.astype(F) / F(n)
    r = round_half_away(mean * scale + bias).astype(np.int64) + z_out
    return np.clip(r, info.min, info.max).astype(x.dtype)


def sqdiff_params(s1, s2, so):
    """(m1, sh1, m2, sh2, mo, sho) of squared_difference.cc's Prepare, or None when the output multiplier is >= 1"""
    t = 2.0 * float(max(F(s1), F(s2)))
    ro = t * t / ((1 << 14) * float(F(so)))
    if not ro < 1.0:
        return None
    return orc.quantize_multiplier(float(F(s1)) / t) + orc.quantize_multiplier(float(F(s2)) / t) + \
        orc.quantize_multiplier(ro)


def np_sqdiff(a, b, s1, z1, s2, z2, so, zo):
    """SQUARED_DIFFERENCE int8 with numpy broadcasting: both inputs << 7 and
    scaled by s / (2 max(s1, s2)), the squared difference scaled by
    (2 max)^2 / (2^14 s_out), + z_out, clamped to [-128, 127]"""
    m1, h1, m2, h2, mo, ho = sqdiff_params(s1, s2, so)
    assert h1 <= 0 and h2 <= 0 and ho <= 0
    xa = rdbypot(srdhm((a.astype(np.int64) - z1) << 7, m1), -h1)
    xb = rdbypot(srdhm((b.astype(np.int64) - z2) << 7, m2), -h2)
    d = xa - xb
    return np.clip(rdbypot(srdhm(d * d, mo), -ho) + zo, -128, 127).astype(np.int8)


def inv_sqrt_multiplier(v):
    """gemmlowp's GetInvSqrtQuantizedMultiplierExp(v, reverse_shift = -1) on a Python int"""
    if v <= 1:
        return (1 << 31) - 1, 0
    shift = 11
    while v >= 1 << 29:
        v //= 4
        shift += 1
    pairs = (31 - v.bit_length()) // 2 - 1  # (clz - 1) / 2 - 1
    shift -= pairs
    v <<= 2 * pairs
    half_in = rdbypot(v >> 1, 1)
    x = 1 << 28  # 1.0 with 3 integer bits
    for _ in range(5):
        x3 = sat_shl(srdhm(srdhm(x, x), x), 6)
        x = sat_shl(srdhm((1 << 28) + (1 << 27), x) - srdhm(half_in, x3), 3)
    x = srdhm(x, 1518500250)
    if shift < 0:
        x <<= -shift
        shift = 0
    return x, -shift


def np_rsqrt_table(s_in, z_in, s_out, z_out):
    """the 256 outputs of int8 RSQRT by input byte (index = the byte as uint8);
    v = q - z_in <= 0 gives 127 (TFLite fails the invoke below zero)"""
    mult, shift = orc.quantize_multiplier(1.0 / float(F(np.sqrt(F(s_in))) * F(s_out)))
    table = np.zeros(256, np.uint8)
    for q in range(-128, 128):
        v, out = q - z_in, 127
        if v > 0:
            m, e = inv_sqrt_multiplier(v)
            data = int(mbqm(1, m, e + 20))
            out = min(max(int(mbqm(data, mult, shift - 20)) + z_out, -128), 127)
        table[q & 0xff] = out & 0xff
    return table


def gelu_real(x, approximate=False):
    """GELU of a Python float in double precision"""
    if approximate:
        return 0.5 * x * (1.0 + math.tanh(0.7978845608028654 * x * (1.0 + 0.044715 * x * x)))
    return 0.5 * x * (1.0 + math.erf(x * 0.7071067811865476))


def gelu_f32_bound(x, ref, ulps):
    """|float32 GELU - ref| allowed at x.  The result is 0.5 x (1 + e) with e =
    erf(x / sqrt 2) or the tanh term, |e| <= 1.  e carries `ulps` ulp of the
    library function (<= ulps 2^-24 absolute) and the rounding of its argument:
    the argument is a product of 2 (erf) or 4 (tanh) float32 operations,
    relative (k + 1) 2^-24, and |u f'(u)| <= 0.5 for both functions (erf: 2 u
    exp(-u^2) / sqrt(pi) <= 0.49; tanh: u sech^2 u <= 0.45), so <= 2.5 2^-24.
    The sum 1 + e adds 2^-24 (its value is at most 2, rounding 2^-24 relative
    would be 2^-23: counted as 2 2^-24).  So |delta(1 + e)| <= (ulps + 4.5)
    2^-24, times 0.5 |x|; the two outer products add 2 2^-24 relative to the
    result, doubled for a compiler that contracts differently; 2^-126 is the
    subnormal floor."""
    x = np.abs(np.asarray(x, np.float64))
    return 0.5 * x * (ulps + 4.5) * 2.0 ** -24 + 4 * 2.0 ** -24 * np.abs(ref) + 2.0 ** -126


def np_gelu_table(signed, approximate, s_in, z_in, s_out, z_out):
    """activations.cc PopulateLookupTable: dequantise in float32, transform (in
    double, rounded to float32 once), round(y * (1 / s_out)), + z_out, clamp"""
    lo, hi = (-128, 127) if signed else (0, 255)
    inv = F(1.0) / F(s_out)
    table = np.zeros(256, np.uint8)
    for q in range(lo, hi + 1):
        x = F(s_in) * F(q - z_in)
        y = F(gelu_real(float(x), approximate))
        r = int(round_half_away(y * inv) + F(z_out))
        table[q & 0xff] = min(max(r, lo), hi) & 0xff
    return table


def lut(x, table):
    return table[x.view(np.uint8)].view(x.dtype)


# ---- cases --------------------------------------------------------------------------------
ROWS_C = [(1, 1), (3, 5), (7, 64), (5, 65), (17, 48), (4, 192), (2, 1000), (3, 4100)]


class MeanCase:
    """rows x C bytes with an all-min row, an all-max row and a row whose sum is
    negative and no multiple of C (int8); `exact`: equal quantisation"""

    def __init__(self, rows, C, dtype, exact, seed=0, offset=0):
        info = np.iinfo(dtype)
        rng = np.random.default_rng(seed + 7 * rows + C)
        self.x = rng.integers(info.min, info.max + 1, (rows, C)).astype(dtype)
        self.x[0] = info.min
        if rows > 1:
            self.x[1] = info.max
        if rows > 2:
            self.x[2] = rng.integers(info.min, info.min + 60, C).astype(dtype)
            if int(self.x[2].astype(np.int64).sum()) % C == 0:
                self.x[2, 0] += 1
        self.dtype, self.exact, self.offset = np.dtype(dtype), exact, offset
        z = -3 if dtype == np.int8 else 125
        self.q_in = (0.05, z)
        self.q_out = (0.05, z) if exact else (0.031, z + 9)
        self.name = "%dx%d_%s_%s%s" % (rows, C, self.dtype.name, "exact" if exact else "rescaled", "_off1" if offset else "")

    def ref(self):
        return np_mean_rows(self.x, *self.q_in, *self.q_out)


def mean_cases():
    cases = [MeanCase(r, c, dt, ex) for (r, c) in ROWS_C for dt in (np.int8, np.uint8) for ex in (True, False)]
    cases += [MeanCase(5, 65, dt, ex, offset=1) for dt in (np.int8, np.uint8) for ex in (True, False)]
    return cases


def mean_params(case, in_ptr, out_ptr):
    from band_amd import _abi
    p = _abi.MeanRowsParams()
    p.rows, p.depth = case.x.shape
    p.type = 1 if case.dtype == np.int8 else 2
    p.exact = int(case.exact)
    scale = F(case.q_in[0]) / F(case.q_out[0])
    p.scale, p.bias, p.out_zp = float(scale), float(F(-case.q_in[1]) * scale + F(0.5)), case.q_out[1]
    p.input, p.output = in_ptr, out_ptr
    return p


def launch_mean(case, lib, device):
    """the case through bh_mean_rows (device) or its host twin; 0xff past the output must stay"""
    from band_amd import _abi
    raw = np.concatenate([np.zeros(case.offset, np.uint8), case.x.view(np.uint8).reshape(-1)])
    n = case.x.shape[0]
    dx, dy = _buffer(raw, device), _buffer(np.full(n + SLACK, 0xff, np.uint8), device)
    p = mean_params(case, dx.value + case.offset, dy.value)
    if device:
        assert lib.bh_mean_rows_kernel(ctypes.byref(p)) == MEAN_KERNEL.encode()
        _abi.check(lib.bh_mean_rows(ctypes.byref(p), None), "bh_mean_rows")
    else:
        assert lib.bhx_cpu_mean_rows(ctypes.byref(p)) == 0, lib.bhx_last_error()
    got = dy.download(np.uint8, (n + SLACK,))
    assert (got[n:] == 0xff).all(), "bytes past the output were written"
    return got[:n].view(case.dtype)


class SqdiffCase:
    def __init__(self, name, sa, sb, q1=(0.05, 3), q2=(0.04, -5), qo=(0.9, -128), seed=0, fill=None):
        rng = np.random.default_rng(seed)
        self.name, self.q1, self.q2, self.qo = name, q1, q2, qo
        self.a = rng.integers(-128, 128, sa).astype(np.int8) if fill is None else np.full(sa, fill[0], np.int8)
        self.b = rng.integers(-128, 128, sb).astype(np.int8) if fill is None else np.full(sb, fill[1], np.int8)

    def ref(self):
        return np_sqdiff(self.a, self.b, *self.q1, *self.q2, *self.qo)


def sqdiff_cases():
    cases = [SqdiffCase("same_3x5x7", (3, 5, 7), (3, 5, 7), seed=1),
             SqdiffCase("row_stats_2x9x48", (2, 9, 48), (2, 9, 1), seed=2),
             SqdiffCase("channel_const_48", (2, 9, 48), (48,), seed=3),
             SqdiffCase("scalar", (2, 9, 48), (1,), seed=4)]
    # the extremes with the largest scale on either side: |a' - b'| is the largest the op can see
    for big in (0, 1):
        q1, q2 = ((0.05, 0), (0.01, 0)) if big == 0 else ((0.01, 0), (0.05, 0))
        for fa, fb in ((-128, 127), (127, -128)):
            cases.append(SqdiffCase("extreme_big%d_%d_%d" % (big, fa, fb), (4, 5), (4, 5), q1=q1, q2=q2, qo=(1.5, -128),
                                    fill=(fa, fb)))
    return cases


def eltwise_params(case, a_ptr, b_ptr, out_ptr):
    from band_amd import _abi
    p = _abi.EltwiseParams()
    p.kind, p.in_signed = 2, 1  # BH_ELT_SQDIFF
    out_shape = np.broadcast_shapes(case.a.shape, case.b.shape)
    for dst, shp in ((p.shape_a, case.a.shape), (p.shape_b, case.b.shape), (p.shape_o, out_shape)):
        for i, v in enumerate((1,) * (4 - len(shp)) + tuple(shp)):
            dst[i] = v
    p.a_off, p.b_off, p.o_off = -case.q1[1], -case.q2[1], case.qo[1]
    p.left_shift = 7
    p.a_mult, p.a_shift, p.b_mult, p.b_shift, p.o_mult, p.o_shift = sqdiff_params(case.q1[0], case.q2[0], case.qo[0])
    p.act_min, p.act_max = -128, 127
    p.a, p.b, p.out = a_ptr, b_ptr, out_ptr
    return p


def launch_sqdiff(case, lib, device):
    from band_amd import _abi
    n = int(np.prod(np.broadcast_shapes(case.a.shape, case.b.shape)))
    da, db = _buffer(case.a.view(np.uint8).reshape(-1), device), _buffer(case.b.view(np.uint8).reshape(-1), device)
    dy = _buffer(np.full(n + SLACK, 0xff, np.uint8), device)
    p = eltwise_params(case, da.value, db.value, dy.value)
    if device:
        _abi.check(lib.bh_eltwise_i8(ctypes.byref(p), None), "bh_eltwise_i8")
    else:
        assert lib.bhx_cpu_eltwise(ctypes.byref(p)) == 0, lib.bhx_last_error()
    got = dy.download(np.uint8, (n + SLACK,))
    assert (got[n:] == 0xff).all(), "bytes past the output were written"
    return got[:n].view(np.int8).reshape(np.broadcast_shapes(case.a.shape, case.b.shape))


# the scales of the table tests: (s_in, z_in, s_out, z_out)
RSQRT_Q = [(0.02, -128, 1.0 / 64, -128), (0.0005, -128, 0.25, -128), (0.3, -100, 0.004, -128)]
GELU_Q = [(True, 0.05, 3, 0.05, -124), (True, 0.02, -7, 0.03, -100), (False, 0.05, 128, 0.05, 4)]


# ---- models ---------------------------------------------------------------------------------
def layer_norm_model(tokens=5, dim=48, batch=1):
    g = QGraph(np.int8, seed=91, name="layer_norm")
    x = g.input([batch, tokens, dim], scale=0.05)
    g.output(g.layer_norm(x))
    return g.build()


LN_OP_OF = {"m": 0, "a": 6}  # which of the ten ops makes the row mean m, the per-element a = x * g


def layer_norm_with_intermediate_output(which):
    """LayerNorm alone on [1, 3, 5] (three rows, depth 5: below every vector width of the kernels) whose
    outputs are y and one intermediate of the pattern, `which` of LN_OP_OF"""
    g = QGraph(np.int8, seed=92, name="layer_norm_out_" + which)
    g.output(g.layer_norm(g.input([1, 3, 5], scale=0.05)))
    g.output(g.mb.ops[-10:][LN_OP_OF[which]]["outputs"][0])
    return g.build()


# ---- the fused launch ------------------------------------------------------------------------
LN_KERNEL = "layernorm_i8_kernel"
LN_MAX_DEPTH = 1024
LN_TEN = [MEAN, SQUARED_DIFFERENCE, MEAN, 0, RSQRT, 18, 18, 18, 41, 0]  # ADD 0, MUL 18, SUB 41


def _elt_block(p, kind, qa, qb, qo, sub=False):
    """one bh_eltwise_params as lower.cc fills it (pointers and shapes unused by the fused kernel)"""
    p.in_signed, p.a_off, p.b_off, p.o_off, p.act_min, p.act_max = 1, -qa[1], -qb[1], qo[1], -128, 127
    for s in (p.shape_a, p.shape_b, p.shape_o):
        for i in range(4):
            s[i] = 1
    if kind == "mul":
        p.kind = 1
        p.o_mult, p.o_shift = orc.mul_params(qa[0], qb[0], qo[0])
    elif kind == "sqdiff":
        p.kind, p.left_shift = 2, 7
        p.a_mult, p.a_shift, p.b_mult, p.b_shift, p.o_mult, p.o_shift = sqdiff_params(qa[0], qb[0], qo[0])
    else:
        m1, s1, m2, s2, mo, so, left = [int(v) for v in orc.add_params(qa[0], qb[0], qo[0])]
        p.kind, p.left_shift = 0, left
        p.a_mult, p.a_shift, p.b_mult, p.b_shift, p.o_mult, p.o_shift = m1, s1, (-m2 if sub else m2), s2, mo, so


def _mean_block(p, depth, q_in, q_out):
    p.rows, p.depth, p.type = 1, depth, 1
    p.exact = int(F(q_in[0]) == F(q_out[0]) and q_in[1] == q_out[1])
    scale = F(q_in[0]) / F(q_out[0])
    p.scale, p.bias, p.out_zp = float(scale), float(F(-q_in[1]) * scale + F(0.5)), q_out[1]


class LnCase:
    """a layer_norm model on [1, rows, C] (its ten ops, quantisation and
    constants), an input, and the ten ops' numpy chain as the expected output"""

    def __init__(self, rows, C, seed=0):
        from oracle.tflite_fb import Model as OModel
        self.rows, self.C, self.name = rows, C, "%dx%d" % (rows, C)
        self.buf = layer_norm_model(tokens=rows, dim=C)
        self.om = OModel(self.buf)
        assert [o.builtin for o in self.om.operators] == LN_TEN
        self.x = model_input(self.buf, seed=seed + rows + C)

    def ref(self):
        from tests.graph_reference import run_reference
        return run_reference(self.buf, self.x)[self.om.outputs[0]].reshape(self.rows, self.C)

    def params(self, in_ptr, gamma_ptr, beta_ptr, table_ptr, out_ptr):
        from band_amd import _abi
        T, ops = self.om.tensors, self.om.operators
        q = lambda t: orc._q(T[t])
        p = _abi.LayerNormParams()
        p.rows, p.depth = self.rows, self.C
        _mean_block(p.mean_x, self.C, q(ops[0].inputs[0]), q(ops[0].outputs[0]))
        _mean_block(p.mean_d, self.C, q(ops[2].inputs[0]), q(ops[2].outputs[0]))
        for blk, k, kind in ((p.sqdiff, 1, "sqdiff"), (p.add_eps, 3, "add"), (p.mul_gamma, 5, "mul"), (p.mul_x, 6, "mul"),
                             (p.mul_m, 7, "mul"), (p.sub_beta, 8, "sub"), (p.add_out, 9, "add")):
            _elt_block(blk, "add" if kind == "sub" else kind, q(ops[k].inputs[0]), q(ops[k].inputs[1]), q(ops[k].outputs[0]),
                       sub=kind == "sub")
        p.eps_q = int(np.asarray(T[ops[3].inputs[1]].data).reshape(-1)[0])
        p.rsqrt_table, p.input, p.gamma, p.beta, p.output = table_ptr, in_ptr, gamma_ptr, beta_ptr, out_ptr
        return p

    def constants(self):
        T, ops = self.om.tensors, self.om.operators
        table = np_rsqrt_table(*orc._q(T[ops[4].inputs[0]]), *orc._q(T[ops[4].outputs[0]]))
        gamma = np.asarray(T[ops[5].inputs[1]].data, np.int8).reshape(-1)
        beta = np.asarray(T[ops[8].inputs[0]].data, np.int8).reshape(-1)
        return table, gamma, beta


def ln_cases():
    return [LnCase(r, c) for r, c in ROWS_C if c <= LN_MAX_DEPTH]


def launch_ln(case, lib, check_only=False):
    """the case through bh_layernorm_i8; 0xff past the output must stay"""
    from band_amd import _abi
    from band_amd.device import DeviceBuffer
    table, gamma, beta = case.constants()
    n = case.rows * case.C
    bufs = [DeviceBuffer.from_array(a.view(np.uint8).reshape(-1)) for a in (case.x, gamma, beta, table)]
    dy = DeviceBuffer.from_array(np.full(n + SLACK, 0xff, np.uint8))
    p = case.params(bufs[0].value, bufs[1].value, bufs[2].value, bufs[3].value, dy.value)
    if check_only:
        return p, bufs + [dy]
    assert lib.bh_layernorm_i8_kernel(ctypes.byref(p)) == LN_KERNEL.encode(), lib.bh_last_error()
    _abi.check(lib.bh_layernorm_i8(ctypes.byref(p), None), "bh_layernorm_i8")
    got = dy.download(np.uint8, (n + SLACK,))
    assert (got[n:] == 0xff).all(), "bytes past the output were written"
    return got[:n].view(np.int8).reshape(case.rows, case.C)


MODELS = {
    "layer_norm_5_48": layer_norm_model,
    "encoder_17_48_3_96": lambda: encoder_block(np.int8, tokens=17, dim=48, heads=3, hidden=96),
    "vit_tiny_32_ln_mlp": lambda: vit_tiny(np.int8, size=32, dim=48, heads=3, layer_norm=True, mlp=True),
}
LAYER_NORMS = {"layer_norm_5_48": 1, "encoder_17_48_3_96": 2, "vit_tiny_32_ln_mlp": 4}


def model_input(buf, seed=0):
    """a random input within +-60 LSB of the zero point: the spread layer_norm calibrates for"""
    from oracle.tflite_fb import Model as OModel
    om = OModel(buf)
    t = om.tensors[om.inputs[0]]
    rng = np.random.default_rng(seed)
    z = int(t.zero_point[0])
    return np.clip(z + np.round(rng.normal(0, 30, t.shape)), -128, 127).astype(np.int8)


def is_encoder_op(om, o):
    """the 8-bit ops restated here: SQUARED_DIFFERENCE, RSQRT, GELU, and MEAN over the last axis
    (8-bit MEAN over H, W and the float forms are the oracle's)"""
    T = om.tensors
    if o.builtin not in (MEAN, SQUARED_DIFFERENCE, RSQRT, GELU) or T[o.inputs[0]].np_dtype not in (np.int8, np.uint8):
        return False
    if o.builtin != MEAN:
        return True
    axes = [int(v) for v in np.asarray(T[o.inputs[1]].data).reshape(-1)]
    return axes in ([-1], [len(T[o.inputs[0]].shape) - 1])


def eval_encoder_op(om, o, vals):
    """operator o (is_encoder_op) on vals"""
    T = om.tensors
    ti, to = T[o.inputs[0]], T[o.outputs[0]]
    x = vals[o.inputs[0]]
    (s_i, z_i), (s_o, z_o) = orc._q(ti), orc._q(to)
    if o.builtin == MEAN:
        return [np_mean_rows(x, s_i, z_i, s_o, z_o).reshape(to.shape)]
    if o.builtin == SQUARED_DIFFERENCE:
        s_b, z_b = orc._q(T[o.inputs[1]])
        return [np_sqdiff(x, vals[o.inputs[1]], s_i, z_i, s_b, z_b, s_o, z_o)]
    if o.builtin == RSQRT:
        assert (x.astype(np.int64) >= z_i).all(), "RSQRT below the zero point"
        return [lut(x, np_rsqrt_table(s_i, z_i, s_o, z_o))]
    approximate = bool(o.options.scalar(0, "b", 0)) if o.options is not None else False
    return [lut(x, np_gelu_table(ti.np_dtype == np.int8, approximate, s_i, z_i, s_o, z_o))]
