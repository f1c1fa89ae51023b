"""Fixtures of grouped CONV_2D (filter [oc, kh, kw, icg] with icg != ic): the
shapes, the cases, the reference, the launcher parameter blocks (host or device
buffers), the models and eval_grouped (one operator for tests.graph_reference).

The reference is the oracle's dense conv per group: output channels
[g ocg, (g+1) ocg) are orc.conv2d of input channels [g icg, (g+1) icg) with
filter rows, bias, multipliers and shifts of the same range, concatenated along
channels (grouped_ref).  The oracle itself does not know groups; an expected
value never comes from the product."""
import ctypes

import numpy as np

from band_amd.tflite_synth import OPT, ModelBuilder, QGraph, conv_options
from oracle import runner as orc
from tests.kernel_harness import ConvCase, dom, rand_q, xor_of

CONV_2D = 3
NONE, RELU6 = 0, 3
MFMA, MFMA_2 = 1, 2  # BH_CONV_GROUPED_MFMA (one pixel tile per wave, the routed form) and BH_CONV_GROUPED_MFMA_2

# (b, ih, iw, G, icg, ocg, kh, kw, stride, dilation, SAME)
SHAPES = [
    (1, 5, 7, 2, 3, 5, 3, 3, 1, 1, True),       # everything odd; ocg % 4 != 0; K_g = 27
    (2, 9, 9, 32, 4, 4, 3, 3, 2, 1, True),      # four groups per 16-channel tile; stride 2; batch 2
    (1, 11, 10, 4, 16, 16, 3, 3, 1, 2, False),  # K_g = 144: two steps and a tail; dilation; aligned slices
    (1, 4, 4, 3, 68, 24, 1, 1, 1, 1, True),     # K_g = 68; 4- but not 16-aligned slices; partial N tile
    (1, 6, 5, 8, 1, 2, 3, 3, 1, 1, True),       # icg = 1
    (3, 17, 13, 2, 20, 18, 3, 3, 1, 1, True),   # M = 663; ocg = 18
    (1, 8, 8, 2, 8, 40, 1, 1, 2, 1, True),      # strided 1x1; ocg > 32
    # beyond the issue's seven: the gather widths those leave out
    (1, 5, 6, 3, 32, 20, 1, 1, 1, 1, True),     # 1x1 with 16-byte slices (ShuffleNet's pointwise at full width)
    (1, 7, 6, 4, 8, 12, 3, 3, 1, 1, True),      # 3x3 with 8-byte slices (ResNeXt 32x4d at 28x28)
]
DTYPES = (np.int8, np.uint8)

# seed of shape i is 100 + i, except where that draw saturates the output:
# (shape, dtype, act) -> a seed whose reference meets the conditions of
# check_reference (found by trying 100 + i + 1000 k for k = 1, 2, ...)
SEED_OVERRIDES = {(2, "uint8", NONE): 1102, (2, "uint8", RELU6): 1102, (8, "uint8", RELU6): 1108}


def forms_for(shape):
    """kernel_hint values whose shape rule admits `shape` (one form in two
    pixel tiles is built, and both take every shape)"""
    return (MFMA, MFMA_2)


def seed_of(i, dtype, act):
    return SEED_OVERRIDES.get((i, np.dtype(dtype).name, act), 100 + i)


class GroupedCase:
    """ConvCase draws the [oc, kh, kw, icg] filter and a quantisation scaled
    for K_g; the [b, ih, iw, G icg] input is drawn after it"""

    def __init__(self, shape, dtype, act=NONE, seed=0, requant_fast=None, hint=0, x=None, **explicit):
        b, ih, iw, G, icg, ocg, kh, kw, s, d, same = shape
        rng = np.random.default_rng(seed)
        self.shape, self.G, self.icg, self.ocg, self.act, self.same = shape, G, icg, ocg, act, same
        self.cc = ConvCase(rng, b, ih, iw, icg, G * ocg, kh, kw, stride=(s, s), dil=(d, d), same=same, dtype=dtype,
                           act=act, requant_fast=requant_fast, kernel_hint=hint, **explicit)
        self.x = rand_q(rng, (b, ih, iw, G * icg), dtype) if x is None else np.ascontiguousarray(x, dtype)
        assert self.x.shape == (b, ih, iw, G * icg)
        self.dtype = dtype
        self.out_shape = (b, self.cc.oh, self.cc.ow, G * ocg)


def grouped_ref(case):
    c = case.cc
    outs = []
    for g in range(case.G):
        sl = slice(g * case.ocg, (g + 1) * case.ocg)
        outs.append(orc.conv2d(
            np.ascontiguousarray(case.x[..., g * case.icg:(g + 1) * case.icg]), np.ascontiguousarray(c.w[sl]),
            np.ascontiguousarray(c.bias[sl]), in_zp=c.in_zp, w_zp=c.w_zp, out_zp=c.out_zp,
            mult=np.ascontiguousarray(c.mult[sl]), shift=np.ascontiguousarray(c.shift[sl]), amin=c.amin, amax=c.amax,
            stride=c.stride, dilation=c.dil, pad=c.pad, out_hw=(c.oh, c.ow)))
    return np.concatenate(outs, axis=3)


def check_reference(case, ref, min_distinct=16):
    """a saturated case cannot pass vacuously: >= 16 distinct bytes, and with
    no activation at least half of them strictly inside the clamp"""
    distinct = len(np.unique(ref))
    inside = float(((ref.astype(np.int32) > case.cc.amin) & (ref.astype(np.int32) < case.cc.amax)).mean())
    assert distinct >= min_distinct, (case.shape, np.dtype(case.dtype).name, distinct)
    if case.act == NONE:
        assert inside >= 0.5, (case.shape, np.dtype(case.dtype).name, inside)
    return distinct, inside


def random_cases():
    """(id, shape index, dtype, act): NONE and RELU6 of every shape x dtype"""
    out = []
    for i in range(len(SHAPES)):
        for dt in DTYPES:
            for act in (NONE, RELU6):
                out.append(("s%d-%s-%s" % (i + 1, np.dtype(dt).name, "none" if act == NONE else "relu6"), i, dt, act))
    return out


def make_case(i, dtype, act, **kw):
    return GroupedCase(SHAPES[i], dtype, act=act, seed=seed_of(i, dtype, act), **kw)


def directed_cases():
    """(id, case) on shapes 1 and 4: the largest accumulators of both signs, a
    per-channel left shift, the input zero point at both ends under SAME padding"""
    out = []
    for i in (0, 3):
        b, ih, iw, G, icg, ocg, kh, kw = SHAPES[i][:8]
        oc, K = G * ocg, kh * kw * icg
        xs, ws = (b, ih, iw, G * icg), (oc, kh, kw, icg)
        # |acc| <= K * 256 * 127 with in_zp at the far end: a multiplier that brings it to ~ +-100
        for name, xv, wv, zp in (("pos", -128, -127, 127), ("neg", -128, 127, 127), ("pos_mirror", 127, 127, -128),
                                 ("neg_mirror", 127, -127, -128)):
            top = K * 255 * 127
            mult, shift = orc.conv_multipliers(1.0, np.full(oc, 100.0 / top, np.float32), oc, 1.0, False)
            out.append(("s%d-extreme-%s" % (i + 1, name), GroupedCase(
                SHAPES[i], np.int8, act=NONE, seed=300 + i, x=np.full(xs, xv, np.int8), w=np.full(ws, wv, np.int8),
                bias=(np.arange(oc, dtype=np.int32) - oc // 2) * 1000, in_zp=zp, out_zp=3, mult=mult, shift=shift,
                amin=-128, amax=127)))
        # per-channel effective multipliers in [1.05, 3.9]: TFLite exponents 1 and 2 (a LEFT shift), on
        # accumulators kept small (x in [-2, 2], w in [-1, 1]: |acc| ~ sqrt(K 4 / 3)) so the output stays inside
        rng = np.random.default_rng(310 + i)
        scales = np.array([2.0 ** (c % 2) * (1.05 + 0.9 * ((c * 7) % 11) / 11.0) for c in range(oc)], np.float32)
        mult, shift = orc.conv_multipliers(1.0, scales, oc, 1.0, False)
        for dt in DTYPES:
            w = rng.integers(-1, 2, ws).astype(np.int16)
            w = w.astype(np.int8) if dt == np.int8 else (w + 128).astype(np.uint8)
            small_x = rng.integers(-2, 3, xs).astype(np.int16)
            x = small_x.astype(np.int8) if dt == np.int8 else (small_x + 128).astype(np.uint8)
            m2, s2 = (mult, shift) if dt == np.int8 else (np.full(oc, mult[1], np.int32), np.full(oc, shift[1], np.int32))
            extra = {} if dt == np.int8 else {"w_zp": 128}
            case = GroupedCase(
                SHAPES[i], dt, act=NONE, seed=320 + i, x=x, w=w, bias=np.arange(oc, dtype=np.int32) % 7 - 3,
                in_zp=0 if dt == np.int8 else 128, out_zp=0 if dt == np.int8 else 128, mult=m2, shift=s2,
                amin=-128 if dt == np.int8 else 0, amax=127 if dt == np.int8 else 255, **extra)
            assert (case.cc.shift > 0).all() and (case.cc.shift == 2).any(), case.cc.shift
            out.append(("s%d-left-shift-%s" % (i + 1, np.dtype(dt).name), case))
        for dt in DTYPES:
            lo, hi = (-128, 127) if dt == np.int8 else (0, 255)
            for zp in (lo, hi):
                out.append(("s%d-in-zp-%d-%s" % (i + 1, zp, np.dtype(dt).name),
                            GroupedCase(SHAPES[i], dt, act=NONE, seed=330 + i, in_zp=zp)))
    return out


# ---- launcher parameter blocks -----------------------------------------------------
class HostBuffer:
    """numpy-backed stand-in for band_amd.device.DeviceBuffer (the CPU entry point)"""

    def __init__(self, a):
        self.a = np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()

    @property
    def value(self):
        return self.a.ctypes.data

    def download(self, dtype, shape):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return self.a[:n].view(dtype).reshape(shape).copy()


def _buffer(a, device):
    if device:
        from band_amd.device import DeviceBuffer
        return DeviceBuffer.from_array(a)
    return HostBuffer(a)


SLACK = 16


def grouped_params(case, lib, keep, device, groups=None):
    """bh_conv_grouped_params of the case; the output buffer is 0xff-filled and SLACK bytes longer than the result"""
    from band_amd import _abi
    c = case.cc
    G = case.G if groups is None else groups
    oc, K = c.oc, c.kh * c.kw * case.icg
    kp, npd = ctypes.c_int(), ctypes.c_int()
    _abi.check(lib.bh_conv_packed_geometry(oc, K, ctypes.byref(kp), ctypes.byref(npd)), "geom")
    packed = np.zeros((npd.value, kp.value), np.int8)
    beff = np.zeros(oc, np.int32)
    wflat = np.ascontiguousarray(c.w.reshape(oc, K))
    bias = np.ascontiguousarray(c.bias, np.int32)
    in_zp_d = dom(c.in_zp, case.dtype)
    w_zp_d = dom(c.w_zp, case.dtype) if case.dtype == np.uint8 else 0
    _abi.check(lib.bh_pack_conv_weights(
        wflat.ctypes.data_as(ctypes.c_void_p), int(case.dtype == np.int8), oc, K, kp.value, npd.value,
        bias.ctypes.data_as(ctypes.c_void_p), in_zp_d, w_zp_d, packed.ctypes.data_as(ctypes.c_void_p),
        beff.ctypes.data_as(ctypes.c_void_p)), "pack")
    m32 = np.ascontiguousarray(c.mult, np.int32)
    s32 = np.ascontiguousarray(c.shift, np.int32)
    nbytes = int(np.prod(case.out_shape))
    bufs = [_buffer(a, device) for a in (case.x, np.full(nbytes + SLACK, 0xff, np.uint8), packed, beff, m32, s32)]
    keep += bufs
    dx, dy, dw, db, dm, ds = bufs
    case._dy = dy
    p = _abi.ConvGroupedParams()
    p.groups = G
    q = p.conv
    q.batch, q.in_h, q.in_w, q.in_c = case.x.shape
    q.out_h, q.out_w, q.out_c = c.oh, c.ow, oc
    q.k_h, q.k_w = c.kh, c.kw
    q.stride_h, q.stride_w = c.stride
    q.dil_h, q.dil_w = c.dil
    q.pad_h, q.pad_w = c.pad
    q.k_pad, q.n_pad, q.in_xor = kp.value, npd.value, xor_of(case.dtype)
    q.in_zp, q.w_zp, q.out_zp, q.act_min, q.act_max = in_zp_d, w_zp_d, c.out_zp, c.amin, c.amax
    q.input, q.output, q.weights, q.bias_eff, q.mult, q.shift = (dx.value, dy.value, dw.value, db.value, dm.value,
                                                                 ds.value)
    fast = lib.bh_conv_requant_fast_ok(m32.ctypes.data_as(ctypes.c_void_p), s32.ctypes.data_as(ctypes.c_void_p), oc, K,
                                       int(np.abs(c.bias.astype(np.int64)).max()))
    q.requant_fast = fast if c.requant_fast is None else int(c.requant_fast and fast)
    q.kernel_hint = c.kernel_hint
    return p


def residual_of(case, ref, seed):
    """a residual tensor, ADD parameters out of TFLite's own Prepare and a byte
    table; returns (r, set(p), expected ADD(ref, r), table)"""
    rng = np.random.default_rng(seed)
    c = case.cc
    signed = case.dtype == np.int8
    r = rand_q(rng, ref.shape, case.dtype)
    r_scale, o_scale = 0.037, 0.051
    r_zp = int(rng.integers(-10, 10)) + (0 if signed else 128)
    o_zp = int(rng.integers(-10, 10)) + (0 if signed else 128)
    prm = orc.add_params(c.out_scale, r_scale, o_scale)
    amin, amax = orc.act_range(1, o_scale, o_zp, signed)  # RELU on the ADD
    z = orc.add(ref, r, a_zp=c.out_zp, b_zp=r_zp, out_zp=o_zp, params=prm, amin=amin, amax=amax)

    def set_add(q, r_ptr):
        q.residual = r_ptr
        q.add_left_shift = int(prm[6])
        q.add_y_off, q.add_r_off, q.add_o_off = -c.out_zp, -r_zp, o_zp
        q.add_y_mult, q.add_y_shift = int(prm[0]), int(prm[1])
        q.add_r_mult, q.add_r_shift = int(prm[2]), int(prm[3])
        q.add_o_mult, q.add_o_shift = int(prm[4]), int(prm[5])
        q.add_act_min, q.add_act_max = amin, amax
    return r, set_add, z, rng.permutation(256).astype(np.uint8)


def check_directed(cid, case, ref):
    """the left-shift cases do shift left (TFLite exponent > 0 on every channel) and do not saturate"""
    if "left-shift" in cid:
        assert (np.asarray(case.cc.shift) > 0).all(), case.cc.shift
        check_reference(case, ref)


def launch(case, lib, device, residual=None, table=None):
    """the case through bh_conv2d_grouped_i8 (device) or its host twin;
    residual = (r, set_add); returns the output and checks the bytes past it"""
    keep = []
    p = grouped_params(case, lib, keep, device)
    if residual is not None:
        dr = _buffer(residual[0], device)
        keep.append(dr)
        residual[1](p.conv, dr.value)
    if table is not None:
        dt = _buffer(table, device)
        keep.append(dt)
        p.conv.out_table = dt.value
    if device:
        from band_amd import _abi
        _abi.check(lib.bh_conv2d_grouped_i8(ctypes.byref(p), None), "bh_conv2d_grouped_i8")
    else:
        assert lib.bhx_cpu_conv_grouped(ctypes.byref(p)) == 0, lib.bhx_last_error()
    n = int(np.prod(case.out_shape))
    got = case._dy.download(np.uint8, (n + SLACK,))
    assert (got[n:] == 0xff).all(), "bytes past the output were written"
    return got[:n].view(case.dtype).reshape(case.out_shape)


# ---- models ------------------------------------------------------------------------
def one_op_model(case, w_shape=None, oc=None):
    """x -> CONV_2D (the case's tensors and quantisation) -> y; w_shape / oc
    override the filter's shape and channel count (refusal models)"""
    c = case.cc
    mb = ModelBuilder("grouped_one_op")
    dt = case.dtype
    x = mb.tensor("x", list(case.x.shape), dt, scale=[c.in_scale], zero_point=[c.in_zp])
    mb.inputs.append(x)
    w = c.w if w_shape is None else np.resize(c.w, w_shape)
    n = w.shape[0]
    if dt == np.int8:
        ws = np.resize(c.w_scales, n).astype(np.float32)
        wt = mb.tensor("w", list(w.shape), np.int8, scale=ws, zero_point=[0] * n, qdim=0, data=w)
    else:
        ws = c.w_scales[:1]
        wt = mb.tensor("w", list(w.shape), np.uint8, scale=ws, zero_point=[c.w_zp], data=w)
    bs = (np.float32(c.in_scale) * (ws if len(ws) > 1 else np.repeat(ws, n))).astype(np.float32)
    bt = mb.tensor("b", [n], np.int32, scale=bs, zero_point=[0] * n, data=np.resize(c.bias, n))
    y = mb.tensor("y", list(case.out_shape[:3]) + [n], dt, scale=[c.out_scale], zero_point=[c.out_zp])
    act = {NONE: "NONE", RELU6: "RELU6"}[case.act]
    mb.op("CONV_2D", [x, wt, bt], [y], OPT["Conv2DOptions"],
          conv_options("SAME" if case.same else "VALID", c.stride[0], act, c.dil[0]))
    mb.outputs.append(y)
    return mb.build()


def float_grouped_model():
    """a float32 CONV_2D whose filter has half the input's channels"""
    mb = ModelBuilder("grouped_float")
    x = mb.tensor("x", [1, 4, 4, 8], np.float32)
    mb.inputs.append(x)
    rng = np.random.default_rng(7)
    w = mb.tensor("w", [6, 1, 1, 4], np.float32, data=rng.uniform(-1, 1, (6, 1, 1, 4)).astype(np.float32))
    b = mb.tensor("b", [6], np.float32, data=np.zeros(6, np.float32))
    y = mb.tensor("y", [1, 4, 4, 6], np.float32)
    mb.op("CONV_2D", [x, w, b], [y], OPT["Conv2DOptions"], conv_options("SAME", 1, "NONE", 1))
    mb.outputs.append(y)
    return mb.build()


def conv_then_add(dtype=np.int8):
    """grouped 3x3 conv -> ADD with the block's input (the fold into the conv's epilogue)"""
    g = QGraph(dtype, seed=71, name="grouped_add")
    x = g.input([1, 9, 7, 12], scale=0.05)
    y = g.conv(x, 12, k=3, act="NONE", groups=3)
    g.output(g.add(y, x))
    return g.build()


def conv_then_relu6(dtype=np.int8):
    """grouped 1x1 conv -> stand-alone RELU6 (the unary-table fold)"""
    g = QGraph(dtype, seed=73, name="grouped_relu6")
    x = g.input([1, 6, 5, 20], scale=0.05)
    y = g.conv(x, 30, k=1, act="NONE", groups=5)
    g.output(g.relu(y, "RELU6"))
    return g.build()


def shufflenet_small(dtype=np.int8):
    """shufflenet_v1 at 32 x 32, width 0.25, one stride-1 unit per stage: small enough for a test"""
    from band_amd.tflite_synth import shufflenet_v1
    return shufflenet_v1(dtype, size=32, width=0.25, classes=10, repeats=(1, 1, 1))


def is_grouped(om, o):
    return (o.builtin == CONV_2D and om.tensors[o.inputs[0]].np_dtype != np.float32 and
            om.tensors[o.inputs[1]].shape[3] != om.tensors[o.inputs[0]].shape[3])


def eval_grouped(om, o, vals):
    """the oracle interpreter's CONV_2D (oracle/runner.py OracleInterpreter._op) per group"""
    T = om.tensors
    opt = o.options
    x, w = vals[o.inputs[0]], vals[o.inputs[1]]
    bias = vals.get(o.inputs[2]) if len(o.inputs) > 2 and o.inputs[2] >= 0 else None
    ti, tw, to = T[o.inputs[0]], T[o.inputs[1]], T[o.outputs[0]]
    same = opt.scalar(0, "b", 0) == 0
    sw, sh = opt.scalar(1, "i", 1), opt.scalar(2, "i", 1)
    act = opt.scalar(3, "b", 0)
    dw_, dh_ = opt.scalar(4, "i", 1), opt.scalar(5, "i", 1)
    oc, kh, kw, icg = w.shape
    G = x.shape[3] // icg
    ocg = oc // G
    ih, iw = x.shape[1], x.shape[2]
    oh, ow = orc.out_size(same, ih, kh, sh, dh_), orc.out_size(same, iw, kw, sw, dw_)
    pad = (orc.padding(sh, dh_, ih, kh, oh), orc.padding(sw, dw_, iw, kw, ow))
    in_s, in_z = orc._q(ti)
    out_s, out_z = orc._q(to)
    legacy = ti.np_dtype == np.uint8
    mult, shift = orc.conv_multipliers(in_s, tw.scale, oc, out_s, legacy)
    amin, amax = orc._act_range_for(act, to)
    w_zp = int(tw.zero_point[0]) if legacy else 0
    outs = []
    for g in range(G):
        sl = slice(g * ocg, (g + 1) * ocg)
        outs.append(orc.conv2d(
            np.ascontiguousarray(x[..., g * icg:(g + 1) * icg]), np.ascontiguousarray(w[sl]),
            None if bias is None else np.ascontiguousarray(bias[sl]), in_zp=in_z, w_zp=w_zp, out_zp=out_z,
            mult=np.ascontiguousarray(mult[sl]), shift=np.ascontiguousarray(shift[sl]), amin=amin, amax=amax,
            stride=(sh, sw), dilation=(dh_, dw_), pad=pad, out_hw=(oh, ow)))
    return [np.concatenate(outs, axis=3)]
