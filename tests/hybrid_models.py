"""Fixtures of the dynamic-range ("hybrid") FULLY_CONNECTED - float32 input,
constant int8 weights with one scale, each input row quantised at run time:
the numpy restatement of the rule, its deliberately wrong variants, the
launcher cases, the models and the rule on one operator of a graph
(hybrid_fc_reference, for tests.float_harness.check_graph_ops).

The rule (DESIGN 4 holds it in words; restated from memory of TFLite's
fully_connected.cc EvalHybrid and tensor_utils::{Symmetric,Asymmetric}
QuantizeFloats, parity unpinned beyond that text).  Every float operation is one
IEEE float32 operation - an explicit .astype(np.float32) after each - and
float64 where marked; round is half away from zero.

  symmetric row x    r = max|x|; r == 0: q = 0, s = 1; else s = r / 127,
                     inv = 127 / r, q = clamp(round(x inv), -127, 127); off = 0
  asymmetric row x   rmin = min(0, min x), rmax = max(0, max x); equal: q = 0,
                     s = 1, off = 0; else (float64) scale = (rmax - rmin) / 255
                     with the difference in float32, z_min = -128 - rmin / scale,
                     z_max = 127 - rmax / scale, e_min = 128 + |rmin / scale|,
                     e_max = 127 + |rmax / scale|, z = e_min < e_max ? z_min : z_max,
                     off = -128 / 127 beyond those, else round(z); s = (float)scale,
                     inv = 1 / s, q = clamp(round((float)off + x inv), -128, 127)
  output             dot = sum_k w[u,k] q_k - off sum_k w[u,k]  (int32, exact)
                     y = bias[u] + (float)dot * (s * ws), clamped to the activation

tests/test_fc_hybrid_cpu.py first judges this restatement alone: against the
float64 product of the dequantised weights at a derived bound, and against its
wrong variants."""
import ctypes
import math

import numpy as np

from band_amd.tflite_synth import FGraph, encoder_block, vit_tiny
from tests import float_harness as H
from tests.fixed_point import round_half_away, round_half_away64

F = np.float32
F64 = np.float64
FULLY_CONNECTED, MEAN = 9, 40
DQ_KERNEL, FC_KERNEL = "dynquant_rows_kernel", "fc_hybrid_kernel"
ACTS = ("NONE", "RELU", "RELU_N1_TO_1", "RELU6")
SLACK = 16  # bytes past every output that a launch must leave alone
NAN_WORD = 0x7fc0dead  # the pattern output buffers are filled with


# ---- the rule ----------------------------------------------------------------------------
def np_dynquant(x, asymmetric, half_even=False):
    """(q int8 [rows][depth], s float32 [rows], off int32 [rows]) of float32 rows x.
    half_even: the wrong variant that rounds ties to even."""
    x = np.asarray(x, F)
    rows, depth = x.shape
    q = np.zeros((rows, depth), np.int8)
    s = np.ones(rows, F)
    off = np.zeros(rows, np.int32)
    rnd = (lambda v: np.rint(v).astype(F)) if half_even else round_half_away
    for i in range(rows):
        row = x[i]
        if not asymmetric:
            r = F(np.abs(row).max())
            if r == 0:
                continue
            s[i] = (r / F(127.0)).astype(F)
            inv = (F(127.0) / r).astype(F)
            t = (row * inv).astype(F)
            q[i] = np.clip(rnd(t).astype(np.int32), -127, 127).astype(np.int8)
            continue
        rmin, rmax = F(min(F(0.0), row.min())), F(max(F(0.0), row.max()))
        if rmin == rmax:
            continue
        rng = (rmax - rmin).astype(F)          # float32
        scale = float(rng) / 255.0             # float64 from here on
        a, b = float(rmin) / scale, float(rmax) / scale
        z_min, z_max = -128.0 - a, 127.0 - b
        e_min, e_max = 128.0 + abs(a), 127.0 + abs(b)
        z = z_min if e_min < e_max else z_max
        o = -128 if z <= -128.0 else (127 if z >= 127.0 else int(round_half_away64(z)))
        off[i] = o
        s[i] = F(scale)
        inv = (F(1.0) / s[i]).astype(F)
        t = (row * inv).astype(F)
        v = (F(o) + t).astype(F)
        q[i] = np.clip(rnd(v).astype(np.int32), -128, 127).astype(np.int8)
    return q, s, off


def np_fc_from_q(q, s, off, w, ws, bias, act="NONE", wrong=None):
    """the output rule on quantised rows.  wrong: "assoc" (dot s) ws, "fma" the
    epilogue as one fused multiply-add, "no_rowsum" the asymmetric row-sum term dropped"""
    w64 = np.asarray(w, np.int8).astype(np.int64)
    dot = q.astype(np.int64) @ w64.T
    if wrong != "no_rowsum":
        dot = dot - off.astype(np.int64)[:, None] * w64.sum(axis=1)[None, :]
    assert np.abs(dot).max(initial=0) < 2 ** 31
    dotf = dot.astype(F)
    b = np.zeros(w64.shape[0], F) if bias is None else np.asarray(bias, F)
    if wrong == "assoc":
        prod = ((dotf * s[:, None]).astype(F) * F(ws)).astype(F)
        y = (b[None, :] + prod).astype(F)
    elif wrong == "fma":
        sc = (s * F(ws)).astype(F)
        y = (b.astype(F64)[None, :] + dotf.astype(F64) * sc.astype(F64)[:, None]).astype(F)
    else:
        sc = (s * F(ws)).astype(F)
        prod = (dotf * sc[:, None]).astype(F)
        y = (b[None, :] + prod).astype(F)
    lo, hi = H.ACT[act]
    return np.minimum(np.maximum(y, F(lo)), F(hi)).astype(F)


def np_fc_hybrid(x, w, ws, bias, act="NONE", asymmetric=False, wrong=None):
    """float32 [rows][units] of float32 rows x, int8 w [units][depth], its scale ws, float32 bias or None"""
    q, s, off = np_dynquant(x, asymmetric, half_even=wrong == "half_even")
    return np_fc_from_q(q, s, off, w, ws, bias, act, wrong)


def real_product(x, w, ws, bias):
    """float64 x . (ws w)^T + bias"""
    y = np.asarray(x, F64) @ (float(F(ws)) * np.asarray(w, np.int8).astype(F64)).T
    return y if bias is None else y + np.asarray(bias, F64)[None, :]


def quantisation_bound(x, w, ws, asymmetric, y):
    """c s ws sum_k |w[u,k]| + gamma(3) |y|: an input value is off its step by at most half a
    step s (symmetric, c = 0.5) or, where the nudged zero point clamps an end value, by a whole
    one (asymmetric, c = 1); the epilogue's three roundings stand behind gamma(3)."""
    _, s, _ = np_dynquant(x, asymmetric)
    c = 1.0 if asymmetric else 0.5
    absw = np.abs(np.asarray(w, np.int8).astype(F64)).sum(axis=1)
    return c * s.astype(F64)[:, None] * float(F(ws)) * absw[None, :] + H.gamma(3) * np.abs(y)


TIE_ROW = np.array([127.0] + [k + 0.5 for k in range(-60, 60)], F)  # inv == 1: 120 ties, 60 of them odd + 0.5


# ---- launcher cases ----------------------------------------------------------------------
class HybridCase:
    """x [rows][depth] float32 (standard normal unless `rows_as`), w uniform in
    +-127 (or `w_fill`), ws = 0.0123.  in_off / q_off / out_off: bytes by which the
    input, the quantised rows and the output are moved off their buffers."""

    def __init__(self, rows, units, depth, asymmetric, bias=True, act="NONE", seed=0, w_fill=None, in_off=0, q_off=0,
                 out_off=0, directed=False, tag=""):
        rng = np.random.default_rng(1000 + seed + 31 * rows + 7 * units + depth)
        self.rows, self.units, self.depth, self.asymmetric, self.act = rows, units, depth, asymmetric, act
        self.x = rng.normal(0, 1, (rows, depth)).astype(F)
        if directed:
            # a zero row between non-zero rows, an all-positive, an all-negative and a constant row
            assert rows >= 6
            self.x[1] = 0
            self.x[2] = np.abs(self.x[2]) + F(0.25)
            self.x[3] = -np.abs(self.x[3]) - F(0.25)
            self.x[4] = F(0.7)
            if depth == TIE_ROW.size:
                self.x[5] = TIE_ROW
        self.w = (rng.integers(-127, 128, (units, depth)) if w_fill is None else np.full((units, depth), w_fill)).astype(np.int8)
        self.ws = 0.0123
        self.bias = rng.normal(0, 1, units).astype(F) if bias else None
        self.in_off, self.q_off, self.out_off = in_off, q_off, out_off
        self.name = "%dx%dx%d_%s%s%s%s" % (rows, units, depth, "asym" if asymmetric else "sym", "" if bias else "_nobias",
                                           "" if act == "NONE" else "_" + act.lower(), tag)

    def quantised(self):
        return np_dynquant(self.x, self.asymmetric)

    def ref(self):
        return np_fc_hybrid(self.x, self.w, self.ws, self.bias, self.act, self.asymmetric)


ROWS = (1, 2, 15, 16, 17, 65)
UNITS = (1, 3, 15, 16, 17, 65)
DEPTHS = (1, 15, 16, 63, 64, 65, 130, 1280)


def launcher_cases():
    """Not the full product: every value of each parameter, every boundary pair of
    rows x units, both forms of the quantisation; depth 64 / 130 / 1280 on 2 rows
    reach the two small-row forms (unit tiles up to depth 128, K slices above),
    17 rows the row-tile form."""
    out, n = [], 0
    for asym in (False, True):
        shapes = [(r, u, 65) for r in (15, 16, 17) for u in (15, 16, 17)]
        shapes += [(r, 17, 130) for r in ROWS] + [(17, u, 63) for u in UNITS] + [(2, u, 130) for u in UNITS]
        shapes += [(2, 33, d) for d in DEPTHS] + [(17, 16, d) for d in DEPTHS] + [(65, 65, 64)]
        for r, u, d in shapes:
            n += 1
            out.append(HybridCase(r, u, d, asym, bias=n % 3 != 0, seed=n))
        for act in ACTS:
            out.append(HybridCase(17, 33, 65, asym, act=act, seed=50))
            out.append(HybridCase(2, 33, 130, asym, act=act, bias=False, seed=51))
        out.append(HybridCase(6, 19, TIE_ROW.size, asym, seed=60, directed=True, tag="_directed"))
        out.append(HybridCase(17, 20, 64, asym, seed=61, directed=True, tag="_directed"))
        for fill in (127, -127):
            out.append(HybridCase(3, 17, 1280, asym, seed=62, w_fill=fill, tag="_w%d" % fill))
            out.append(HybridCase(18, 17, 1280, asym, seed=63, w_fill=fill, tag="_w%d" % fill))
        # pointers 4 bytes off their buffers: scalar loads, dword fragments, dword stores
        for r, u, d in ((2, 16, 64), (17, 16, 64), (17, 20, 130), (3, 8, 1280)):
            out.append(HybridCase(r, u, d, asym, seed=64, in_off=4, q_off=4, out_off=4, tag="_off4"))
    return out


class AlignedHost:
    """64-byte aligned numpy bytes with DeviceBuffer's interface (the CPU entry points)"""

    def __init__(self, a):
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        self.store = np.zeros(raw.size + 64, np.uint8)
        self.shift = (-self.store.ctypes.data) % 64
        self.a = self.store[self.shift:self.shift + raw.size]
        self.a[...] = raw

    @property
    def value(self):
        return self.a.ctypes.data

    def download(self, dtype, shape):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return self.a[:n].view(dtype).reshape(shape).copy()


def buffer(a, device):
    if device:
        from band_amd.device import DeviceBuffer
        return DeviceBuffer.from_array(np.ascontiguousarray(a).view(np.uint8).reshape(-1))
    return AlignedHost(a)


def pack_weights(w):
    """([units][depth_pad] int8 with zero padding, depth_pad, row sums int32)"""
    units, depth = w.shape
    depth_pad = (depth + 15) // 16 * 16
    packed = np.zeros((units, depth_pad), np.int8)
    packed[:, :depth] = w
    return packed, depth_pad, w.astype(np.int64).sum(axis=1).astype(np.int32)


def _filled(nbytes, word):
    return np.full((nbytes + 3) // 4, word, np.uint32).view(np.uint8)[:nbytes].copy()


def launch(case, lib, device):
    """The case through bh_dynquant_rows + bh_fc_hybrid (device) or their host
    twins, the kernel names asserted first.  Every output lies in a buffer filled
    with a pattern (NaN words for the floats) whose SLACK trailing bytes, and the
    bytes in front of a moved pointer, must stay.  Returns (q, s, off, y)."""
    from band_amd import _abi
    r, u, d = case.rows, case.units, case.depth
    packed, depth_pad, sums = pack_weights(case.w)
    keep = []

    def out_buf(nbytes, off, word):
        b = buffer(_filled(off + nbytes + SLACK, word), device)
        keep.append(b)
        return b

    dx = buffer(np.concatenate([np.zeros(case.in_off, np.uint8), case.x.view(np.uint8).reshape(-1)]), device)
    dq = out_buf(r * d, case.q_off, 0xa5a5a5a5)
    ds, do = out_buf(4 * r, 0, NAN_WORD), out_buf(4 * r, 0, 0xa5a5a5a5)
    dy = out_buf(4 * r * u, case.out_off, NAN_WORD)
    dw, dsum = buffer(packed, device), buffer(sums, device)
    db = buffer(case.bias, device) if case.bias is not None else None
    keep += [dx, dw, dsum, db]
    p = _abi.DynQuantParams()
    p.rows, p.depth, p.asymmetric = r, d, int(case.asymmetric)
    p.input, p.q, p.scale, p.offset = dx.value + case.in_off, dq.value + case.q_off, ds.value, do.value
    f = _abi.FcHybridParams()
    f.rows, f.depth, f.depth_pad, f.units = r, d, depth_pad, u
    f.w_scale = case.ws
    f.act_min, f.act_max = H.ACT[case.act]
    f.q, f.in_scale, f.in_offset = p.q, p.scale, p.offset
    f.weights, f.w_row_sum, f.bias = dw.value, dsum.value, db.value if db is not None else None
    f.output = dy.value + case.out_off
    if device:
        assert lib.bh_dynquant_rows_kernel(ctypes.byref(p)) == DQ_KERNEL.encode(), lib.bh_last_error()
        _abi.check(lib.bh_dynquant_rows(ctypes.byref(p), None), "bh_dynquant_rows")
        assert lib.bh_fc_hybrid_kernel(ctypes.byref(f)) == FC_KERNEL.encode(), lib.bh_last_error()
        _abi.check(lib.bh_fc_hybrid(ctypes.byref(f), None), "bh_fc_hybrid")
    else:
        assert lib.bh_dynquant_rows_kernel(ctypes.byref(p)) == DQ_KERNEL.encode(), lib.bh_last_error()
        assert lib.bhx_cpu_dynquant_rows(ctypes.byref(p)) == 0, lib.bhx_last_error()
        assert lib.bh_fc_hybrid_kernel(ctypes.byref(f)) == FC_KERNEL.encode(), lib.bh_last_error()
        assert lib.bhx_cpu_fc_hybrid(ctypes.byref(f)) == 0, lib.bhx_last_error()

    def take(buf, nbytes, off, word, dtype, shape):
        got = buf.download(np.uint8, (off + nbytes + SLACK,))
        fill = _filled(off + nbytes + SLACK, word)
        assert (got[:off] == fill[:off]).all(), "bytes in front of the output were written"
        assert (got[off + nbytes:] == fill[off + nbytes:]).all(), "bytes past the output were written"
        return got[off:off + nbytes].copy().view(dtype).reshape(shape)

    q = take(dq, r * d, case.q_off, 0xa5a5a5a5, np.int8, (r, d))
    s = take(ds, 4 * r, 0, NAN_WORD, F, (r,))
    off = take(do, 4 * r, 0, 0xa5a5a5a5, np.int32, (r,))
    y = take(dy, 4 * r * u, case.out_off, NAN_WORD, F, (r, u))
    return q, s, off, y


def valid_blocks(ptr):
    """(DynQuantParams, FcHybridParams) the checks accept, every pointer `ptr` (16-byte aligned)"""
    from band_amd import _abi
    p = _abi.DynQuantParams()
    p.rows, p.depth, p.asymmetric = 3, 40, 0
    p.input = p.q = p.scale = p.offset = ptr
    f = _abi.FcHybridParams()
    f.rows, f.depth, f.depth_pad, f.units = 3, 40, 48, 5
    f.w_scale, f.act_min, f.act_max = 0.01, -math.inf, math.inf
    f.q = f.in_scale = f.in_offset = f.weights = f.w_row_sum = f.bias = f.output = ptr
    return p, f


# (name, which block, the change, the reason)
DQ_REFUSALS = [("null_input", dict(input=None), "null pointer"), ("null_q", dict(q=None), "null pointer"),
               ("zero_rows", dict(rows=0), "non-positive extent"), ("negative_depth", dict(depth=-1), "non-positive extent"),
               ("elements", dict(rows=1 << 20, depth=1 << 11), "2^31 or more elements")]
FC_REFUSALS = [("null_weights", dict(weights=None), "null pointer"), ("null_output", dict(output=None), "null pointer"),
               ("zero_units", dict(units=0), "non-positive extent"), ("zero_rows", dict(rows=0), "non-positive extent"),
               ("depth", dict(depth=65536, depth_pad=65536), "depth > 65,535"),
               ("elements", dict(rows=1 << 20, units=1 << 11), "2^31 or more elements"),
               ("depth_pad", dict(depth_pad=40), "depth_pad")]


# ---- models ------------------------------------------------------------------------------
def one_op_model(rows_shape, units, hybrid, act="NONE", keep_num_dims=False, bias=True, seed=70):
    """one hybrid FULLY_CONNECTED on an input of shape rows_shape"""
    g = FGraph(seed=seed, name="hybrid_fc")
    x = g.input(list(rows_shape))
    y = g.fully_connected(x, units, act=act, keep_num_dims=keep_num_dims, hybrid=hybrid)
    if not bias:
        g.mb.ops[-1]["inputs"] = g.mb.ops[-1]["inputs"][:2]
    g.output(y)
    return g.build()


ENCODER_SHAPES = ((17, 48, 3, 96), (64, 64, 2, 128))  # (tokens, dim, heads, hidden)


def _encoder(shape, hybrid):
    t, c, h, hid = shape
    return lambda: encoder_block(np.float32, tokens=t, dim=c, heads=h, hidden=hid, hybrid=hybrid)


MODELS = {}
for _hy in ("symmetric", "asymmetric"):
    MODELS["fc_1x130_to_33_%s" % _hy] = (lambda hy=_hy: one_op_model((1, 130), 33, hy, act="RELU"))
    MODELS["fc_1x17x48_to_20_keep_%s" % _hy] = (lambda hy=_hy: one_op_model((1, 17, 48), 20, hy, keep_num_dims=True,
                                                                            bias=False))
    for _s in ENCODER_SHAPES:
        MODELS["encoder_%d_%d_%d_%d_%s" % (_s + (_hy,))] = _encoder(_s, _hy)
MODELS["vit_tiny_32_symmetric"] = lambda: vit_tiny(np.float32, size=32, dim=48, heads=3, layer_norm=True, mlp=True,
                                                   hybrid="symmetric")
MODELS["vit_tiny_32_asymmetric"] = lambda: vit_tiny(np.float32, size=32, dim=48, heads=3, layer_norm=True, mlp=True,
                                                    blocks=1, hybrid="asymmetric")
REGISTRATION = "encoder_17_48_3_96_symmetric"  # the model of the registration test
BATCHED = "encoder_17_48_3_96_asymmetric"      # the model of the job-batch and engine tests


def model_feed(buf, seed=0):
    from oracle.tflite_fb import Model as OModel
    om = OModel(buf)
    rng = np.random.default_rng(seed)
    return {t: rng.normal(0, 1, om.tensors[t].shape).astype(F) for t in om.inputs}


def is_hybrid_fc(om, o):
    return o.builtin == FULLY_CONNECTED and om.tensors[o.inputs[1]].np_dtype == np.int8


def hybrid_fc_reference(om, o, x):
    """np_fc_hybrid of operator o on input x (the executor's own)"""
    T = om.tensors
    w = T[o.inputs[1]]
    assert len(w.scale) == 1 and int(w.zero_point[0]) == 0
    bias = T[o.inputs[2]].data if len(o.inputs) > 2 and o.inputs[2] >= 0 else None
    opt = o.options
    act = ACTS[opt.scalar(0, "b", 0)] if opt is not None else "NONE"
    asym = bool(opt.scalar(3, "b", 0)) if opt is not None else False
    depth = w.shape[1]
    y = np_fc_hybrid(np.asarray(x, F).reshape(-1, depth), w.data, float(w.scale[0]), bias, act, asym)
    return y.reshape(T[o.outputs[0]].shape)
