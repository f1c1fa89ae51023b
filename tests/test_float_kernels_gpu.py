"""Op-level parity of the float32 kernels (band_amd/csrc/kernels/float_ops.hip)
through the C ABI, against float64 references at the derived per-element
bounds of tests/float_harness.py: tiny shapes at every tail, border and
split-K path, non-finite values, and the float graphs op by op on the GPU
worker (the cases of tests/test_float_ops_cpu.py)."""
import ctypes

import numpy as np
import pytest

from tests import float_harness as H
from tests.glue_models import float_edge_zoo, float_zoo
from tests.test_float_ops_cpu import check_all_ops, check_outputs_only, graph_feed, nonfinite_feed

pytestmark = pytest.mark.gpu

f32 = np.float32
ACTS = ("NONE", "RELU", "RELU6", "RELU_N1_TO_1")


def act_input(rng, shape, positive=False):
    """uniform(-1, 1) + 0.5 (a padding or border mistake cannot cancel); positive: uniform(0.1, 2.1)"""
    return (rng.uniform(-1, 1, shape) + (1.1 if positive else 0.5)).astype(f32)


def weights(rng, shape):
    return rng.standard_normal(shape).astype(f32)


# ---- launch helpers --------------------------------------------------------
def _dev(a):
    from band_amd.device import DeviceBuffer
    return DeviceBuffer.from_array(np.ascontiguousarray(a, f32))


def _out(n):
    from band_amd.device import DeviceBuffer
    b = DeviceBuffer(4 * n)
    b.upload(np.full(n, 7777.0, f32))  # a value no case produces: an unwritten element shows
    return b


def conv_params(x, w, g, act, dm=None):
    from band_amd import _abi
    n, ih, iw, ic = x.shape
    oc = w.shape[3] if dm else w.shape[0]
    lo, hi = H.ACT[act]
    return _abi.ConvF32Params(batch=n, in_h=ih, in_w=iw, in_c=ic, out_h=g.out_hw[0], out_w=g.out_hw[1], out_c=oc,
                              k_h=g.k_hw[0], k_w=g.k_hw[1], stride_h=g.stride[0], stride_w=g.stride[1],
                              dil_h=g.dilation[0], dil_w=g.dilation[1], pad_h=g.pad[0], pad_w=g.pad[1],
                              depthwise=1 if dm else 0, depth_multiplier=dm or 1, act_min=lo, act_max=hi)


def run_conv(lib, x, w, bias, g, act, dm=None):
    """w OHWI (conv) or [1,KH,KW,C*dm] (depthwise); the kernels read [K][out_c]"""
    from band_amd import _abi
    p = conv_params(x, w, g, act, dm)
    laid = w.reshape(-1, p.out_c) if dm else w.reshape(p.out_c, -1).T
    dx, dw_, dy = _dev(x), _dev(laid), _out(x.shape[0] * g.out_hw[0] * g.out_hw[1] * p.out_c)
    db = _dev(bias) if bias is not None else None
    p.input, p.weights, p.output, p.bias = dx.value, dw_.value, dy.value, db.value if db else None
    _abi.check(lib.bh_conv2d_f32(ctypes.byref(p), None), "bh_conv2d_f32")
    return dy.download(f32, (x.shape[0], g.out_hw[0], g.out_hw[1], p.out_c))


def run_fc(lib, x, w, bias, act):
    from band_amd import _abi
    rows, (units, depth) = x.shape[0], w.shape
    lo, hi = H.ACT[act]
    dx, dw_, dy = _dev(x), _dev(w), _out(rows * units)
    db = _dev(bias) if bias is not None else None
    p = _abi.FcF32Params(rows=rows, depth=depth, units=units, act_min=lo, act_max=hi, input=dx.value,
                         output=dy.value, weights=dw_.value, bias=db.value if db else None)
    _abi.check(lib.bh_fc_f32(ctypes.byref(p), None), "bh_fc_f32")
    return dy.download(f32, (rows, units))


def run_eltwise(lib, a, b, kind, act):
    from band_amd import _abi
    so = np.broadcast_shapes(a.shape, b.shape)
    lo, hi = H.ACT[act]
    da, db, dy = _dev(a), _dev(b), _out(int(np.prod(so)))
    p = _abi.EltwiseF32Params(kind={"add": 0, "sub": 1, "mul": 2, "sqdiff": 3}[kind], act_min=lo, act_max=hi,
                              a=da.value, b=db.value, out=dy.value)
    p.shape_a[:], p.shape_b[:], p.shape_o[:] = a.shape, b.shape, so
    _abi.check(lib.bh_eltwise_f32(ctypes.byref(p), None), "bh_eltwise_f32")
    return dy.download(f32, so)


def run_pool(lib, x, kind, g, act):
    from band_amd import _abi
    n, ih, iw, c = x.shape
    lo, hi = H.ACT[act]
    dx, dy = _dev(x), _out(n * g.out_hw[0] * g.out_hw[1] * c)
    p = _abi.PoolF32Params(kind=0 if kind == "avg" else 1, batch=n, in_h=ih, in_w=iw, channels=c,
                           out_h=g.out_hw[0], out_w=g.out_hw[1], f_h=g.k_hw[0], f_w=g.k_hw[1],
                           stride_h=g.stride[0], stride_w=g.stride[1], pad_h=g.pad[0], pad_w=g.pad[1],
                           act_min=lo, act_max=hi, input=dx.value, output=dy.value)
    _abi.check(lib.bh_pool_f32(ctypes.byref(p), None), "bh_pool_f32")
    return dy.download(f32, (n, g.out_hw[0], g.out_hw[1], c))


def run_unary(lib, kind, x, lo=0.0, hi=0.0):
    from band_amd import _abi
    dx, dy = _dev(x), _out(x.size)
    _abi.check(lib.bh_unary_f32({"clamp": 0, "logistic": 1, "rsqrt": 2}[kind], dx.value, dy.value, x.size, lo, hi,
                                None), "bh_unary_f32")
    return dy.download(f32, x.shape)


def run_softmax(lib, x, beta):
    from band_amd import _abi
    dx, dy = _dev(x), _out(x.size)
    _abi.check(lib.bh_softmax_f32(dx.value, dy.value, x.shape[0], x.shape[1], beta, None), "bh_softmax_f32")
    return dy.download(f32, x.shape)


# ---- conv_f32_kernel -------------------------------------------------------
# (b, h, w, ic, oc, k_h, k_w, stride, dilation, SAME, the split-K factor the launcher takes)
CONV_CASES = {
    "k27_tail_asym_pad": (2, 5, 7, 3, 5, 3, 3, 2, 1, True, 1),    # out_c % 4 tail, SAME stride 2: asymmetric pad
    "k63_ks2_midtap": (1, 6, 5, 7, 8, 3, 3, 1, 1, True, 2),       # slice 1 starts at k 32 = tap 4, channel 4
    "k117_ks4": (1, 5, 5, 13, 6, 3, 3, 1, 1, True, 4),
    "k129_ks8_ragged": (1, 9, 9, 129, 3, 1, 1, 1, 1, True, 8),    # K % ks != 0
    "k360_ks16": (1, 5, 4, 40, 12, 3, 3, 1, 1, True, 16),
    "all_taps_clipped": (1, 3, 3, 4, 4, 5, 5, 1, 1, True, 4),     # 3x3 input under a 5x5 kernel
    "dilation2_valid": (1, 9, 8, 3, 4, 3, 3, 1, 2, False, 1),
    "oc1": (1, 4, 5, 6, 1, 3, 3, 1, 1, True, 2),
    "oc2": (1, 4, 5, 6, 2, 3, 3, 1, 1, True, 2),
    "oc3_stride2_valid": (2, 7, 6, 6, 3, 3, 2, 2, 1, False, 2),
    "large_grid_ks1": (4, 64, 64, 8, 64, 3, 3, 1, 1, True, 1),    # 1024 workgroups: no split although K 72 >= 64
}


def conv_case(name):
    b, h, w, ic, oc, kh, kw, stride, dil, same, ks = CONV_CASES[name]
    rng = np.random.default_rng(sorted(CONV_CASES).index(name) + 100)
    x = act_input(rng, (b, h, w, ic), positive=name == "k117_ks4")
    return x, weights(rng, (oc, kh, kw, ic)), weights(rng, oc), H.Geom((h, w), (kh, kw), stride, dil, same), ks


def test_conv_cases_cover_every_split(gpu_lib):
    """every split-K factor of bh_conv2d_f32 is taken by a case below, as bh_conv2d_f32_split reports it"""
    taken, ragged = {}, set()
    for name in CONV_CASES:
        x, w, _, g, ks = conv_case(name)
        p = conv_params(x, w, g, "NONE")
        taken[name] = gpu_lib.bh_conv2d_f32_split(ctypes.byref(p))
        assert taken[name] == ks, (name, taken[name])
        total = x.shape[0] * g.out_hw[0] * g.out_hw[1] * ((w.shape[0] + 3) // 4)
        if ks > 1 and total % (256 // ks) != 0:
            ragged.add(ks)  # dead items behind the barrier
    assert set(taken.values()) == {1, 2, 4, 8, 16}
    assert ragged == {2, 4, 8, 16}
    p.depthwise = 1
    assert gpu_lib.bh_conv2d_f32_split(ctypes.byref(p)) == 0 and gpu_lib.bh_conv2d_f32_split(None) == 0


@pytest.mark.parametrize("name", sorted(CONV_CASES))
def test_conv_f32(gpu_lib, name):
    x, w, bias, g, _ = conv_case(name)
    big = name == "large_grid_ks1"
    combos = [(None, "NONE"), (bias, "RELU6")] if big else [(b_, a) for b_ in (None, bias) for a in ACTS]
    for b_, act in combos:
        ref, tol = H.conv_ref(x, w, b_, g, H.ACT[act])
        if act != "NONE" and w[0].size >= 63 and ref.size >= 64:  # K >= 63: the data reaches both bounds
            assert ref.min() == H.ACT[act][0] and (ref.max() == H.ACT[act][1] or act == "RELU"), (name, act)
        H.check(run_conv(gpu_lib, x, w, b_, g, act), ref, tol,
                "conv_f32_kernel %s bias %s %s" % (name, b_ is not None, act))


# ---- dwconv_f32_kernel -----------------------------------------------------
# (b, h, w, ic, dm, k, stride, dilation, SAME): out_c 5, 6, 9, 12 - 4-channel groups that straddle input channels
DW_CASES = [(3, 7, 5, 5, 1, 3, 1, 1, True), (3, 7, 5, 3, 2, 3, 2, 1, True), (3, 9, 7, 3, 3, 5, 1, 1, True),
            (3, 9, 7, 4, 3, 3, 1, 2, False), (3, 7, 9, 6, 2, 5, 2, 1, False), (1, 5, 5, 6, 1, 3, 2, 1, False),
            (2, 3, 3, 3, 3, 5, 1, 1, True), (3, 8, 6, 4, 3, 3, 2, 2, True)]


@pytest.mark.parametrize("case", DW_CASES, ids=lambda c: "x".join(map(str, c)))
def test_dwconv_f32(gpu_lib, case):
    b, h, w_, ic, dm, k, stride, dil, same = case
    rng = np.random.default_rng(200 + sum(case))
    x = act_input(rng, (b, h, w_, ic), positive=dm == 2)
    w, bias = weights(rng, (1, k, k, ic * dm)), weights(rng, ic * dm)
    g = H.Geom((h, w_), (k, k), stride, dil, same)
    for b_, act in [(None, "NONE"), (bias, "NONE"), (bias, "RELU"), (bias, "RELU6"), (None, "RELU_N1_TO_1")]:
        ref, tol = H.conv_ref(x, w, b_, g, H.ACT[act], depth_multiplier=dm)
        H.check(run_conv(gpu_lib, x, w, b_, g, act, dm=dm), ref, tol,
                "dwconv_f32_kernel %s bias %s %s" % (case, b_ is not None, act))


# ---- fc_f32_kernel ---------------------------------------------------------
@pytest.mark.parametrize("units", [1, 9, 1001])
@pytest.mark.parametrize("depth", [1, 37, 64, 65, 1280])
def test_fc_f32(gpu_lib, depth, units):
    rng = np.random.default_rng(300 + depth + units)
    w, bias = weights(rng, (units, depth)), weights(rng, units)
    for rows in (1, 3):  # rows * units % 4 != 0 for units 1, 9, 1001
        x = act_input(rng, (rows, depth), positive=rows == 3)
        for b_, act in [(None, "NONE"), (bias, "NONE"), (bias, "RELU6"), (None, "RELU_N1_TO_1")]:
            ref, tol = H.fc_ref(x, w, b_, H.ACT[act])
            H.check(run_fc(gpu_lib, x, w, b_, act), ref, tol,
                    "fc_f32_kernel rows %d depth %d units %d bias %s %s" % (rows, depth, units, b_ is not None, act))


# ---- eltwise_f32_kernel ----------------------------------------------------
FULL = (2, 5, 7, 6)  # 420 elements: n % 256 != 0
ELT_SHAPES = [(FULL, FULL), (FULL, (1, 5, 7, 6)), (FULL, (2, 1, 7, 6)), (FULL, (2, 5, 1, 6)), (FULL, (2, 5, 7, 1)),
              (FULL, (1, 1, 1, 6)), (FULL, (1, 1, 1, 1)), ((1, 1, 1, 6), FULL), ((2, 1, 1, 1), FULL),
              ((1, 5, 1, 6), (2, 1, 7, 1))]


@pytest.mark.parametrize("kind", ["add", "sub", "mul", "sqdiff"])
def test_eltwise_f32(gpu_lib, kind):
    rng = np.random.default_rng(400)
    for i, (sa, sb) in enumerate(ELT_SHAPES):
        a, b = act_input(rng, sa, positive=i == 1), (4.0 * weights(rng, sb)).astype(f32)
        for act in ("NONE", "RELU_N1_TO_1") if i < 2 else ("RELU6",) if i == 2 else ("NONE",):
            ref, tol = H.eltwise_ref(a, b, kind, H.ACT[act])
            if act != "NONE":  # the data reaches both bounds (a squared difference has no negative side)
                assert ref.max() == H.ACT[act][1] and (kind == "sqdiff" or ref.min() == H.ACT[act][0])
            H.check(run_eltwise(gpu_lib, a, b, kind, act), ref, tol,
                    "eltwise_f32_kernel %s a %s b %s %s" % (kind, sa, sb, act))


# ---- pool_f32_kernel -------------------------------------------------------
# (b, h, w, c, f_h, f_w, stride, SAME)
POOL_CASES = [(2, 7, 5, 3, 3, 3, 2, True),    # SAME, pad 1: windows clipped on every side
              (1, 5, 6, 1, 4, 4, 1, True),    # 4x4 filter: pad 1 before, 2 after
              (2, 9, 8, 5, 2, 2, 3, False),   # stride larger than the filter
              (2, 6, 5, 7, 6, 5, 1, False),   # global pool
              (1, 1, 9, 3, 1, 4, 2, True)]


@pytest.mark.parametrize("kind", ["avg", "max"])
@pytest.mark.parametrize("case", POOL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_pool_f32(gpu_lib, case, kind):
    b, h, w_, c, fh, fw, stride, same = case
    rng = np.random.default_rng(500 + sum(case[:7]))
    g = H.Geom((h, w_), (fh, fw), stride, 1, same)
    for data in ("offset", "positive", "negative"):
        x = act_input(rng, (b, h, w_, c), positive=data != "offset")
        x = -x if data == "negative" else x  # a maximum over all-negative data
        for act in ("NONE", "RELU6") if data == "offset" else ("NONE",):
            ref, tol = H.pool_ref(4 * x, kind, g, H.ACT[act])
            H.check(run_pool(gpu_lib, 4 * x, kind, g, act), ref, tol,
                    "pool_f32_kernel %s %s %s %s" % (kind, case, data, act))


# ---- unary_f32_kernel ------------------------------------------------------
def test_unary_clamp_f32(gpu_lib):
    x = np.concatenate([np.linspace(-8, 8, 1001), [0.0, -0.0, 1.0, -1.0, 6.0]]).astype(f32)
    for name in ("RELU", "RELU6", "RELU_N1_TO_1"):
        lo, hi = H.ACT[name]
        H.check(run_unary(gpu_lib, "clamp", x, lo, hi), *H.clamp_ref(x, lo, hi), "unary_f32_kernel clamp " + name)


def test_unary_logistic_f32(gpu_lib):
    x = np.concatenate([np.linspace(-100, 100, 4001), [0.0, -0.0], np.linspace(0.01, 20, 700)]).astype(f32)
    assert x.size % 256 != 0
    H.check(run_unary(gpu_lib, "logistic", x), *H.logistic_ref(x), "unary_f32_kernel logistic")


def test_unary_rsqrt_f32(gpu_lib):
    x = np.concatenate([np.logspace(-6, 6, 1201), [0.0, 1.0, 4.0]]).astype(f32)  # 12 decades; 0 gives +inf
    ref, tol = H.rsqrt_ref(x)
    assert np.isposinf(ref[1201])
    H.check(run_unary(gpu_lib, "rsqrt", x), ref, tol, "unary_f32_kernel rsqrt")


# ---- softmax_f32_kernel ----------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2, 63, 64, 65, 1001])
def test_softmax_f32(gpu_lib, depth):
    rng = np.random.default_rng(600 + depth)
    for rows in (1, 5, 9):  # 5 and 9: not a multiple of the 4 waves of a workgroup
        x = (4 * act_input(rng, (rows, depth), positive=rows == 5)).astype(f32)
        if rows == 5 and depth > 64:
            x[2, depth - 1] += 300.0  # the maximum in a lane's second pass: a missed one overflows expf
        if rows == 9:
            x[3] = 1.25  # a constant row
            if depth > 1:
                x[6, 1:] = x[6, 0] - 200.0  # expf underflows: the reference is below 2^-126, 0 is accepted
        for beta in (1.0, 0.8, 3.0):
            ref, tol = H.softmax_ref(x, f32(beta))
            H.check(run_softmax(gpu_lib, x, beta), ref, tol,
                    "softmax_f32_kernel rows %d depth %d beta %g" % (rows, depth, beta))


# ---- non-finite values -----------------------------------------------------
# NaN and +-inf must come out where TFLite's std::min(std::max(v, lo), hi)
# and the kCPU worker's ClampF put them (tests/test_float_ops_cpu.py holds the
# CPU worker to the same float64 model): a NaN stays NaN through a fused
# activation, +inf clamps to the upper bound, -inf to the lower.
def plant(x):
    """+inf, -inf and NaN at three positions of each image, far enough apart
    that small windows see one of them at most"""
    flat = x.reshape(x.shape[0], -1)
    n = flat.shape[1]
    flat[:, 1], flat[:, n // 2], flat[:, n - 2] = np.inf, -np.inf, np.nan
    return x


NONFINITE_ACTS = ("NONE", "RELU6")


def test_nonfinite_conv(gpu_lib):
    rng = np.random.default_rng(700)
    x = plant(act_input(rng, (2, 9, 9, 4)))
    w, bias = weights(rng, (6, 3, 3, 4)), weights(rng, 6)
    g = H.Geom((9, 9), (3, 3), 1, 1, True)
    for act in NONFINITE_ACTS:
        ref, tol = H.conv_ref(x, w, bias, g, H.ACT[act])
        assert np.isnan(ref).any() and (act != "NONE" or (np.isposinf(ref).any() and np.isneginf(ref).any()))
        H.check(run_conv(gpu_lib, x, w, bias, g, act), ref, tol, "non-finite conv_f32_kernel " + act)


def test_nonfinite_dwconv(gpu_lib):
    rng = np.random.default_rng(701)
    x = plant(act_input(rng, (2, 9, 9, 3)))
    w, bias = weights(rng, (1, 3, 3, 6)), weights(rng, 6)
    g = H.Geom((9, 9), (3, 3), 1, 1, True)
    for act in NONFINITE_ACTS:
        ref, tol = H.conv_ref(x, w, bias, g, H.ACT[act], depth_multiplier=2)
        assert np.isnan(ref).any()
        H.check(run_conv(gpu_lib, x, w, bias, g, act, dm=2), ref, tol, "non-finite dwconv_f32_kernel " + act)


def test_nonfinite_fc(gpu_lib):
    rng = np.random.default_rng(702)
    x = act_input(rng, (4, 70))
    x[0, 3], x[1, 69], x[2, 64] = np.inf, -np.inf, np.nan  # row 3 stays finite
    w, bias = weights(rng, (9, 70)), weights(rng, 9)
    for act in NONFINITE_ACTS:
        ref, tol = H.fc_ref(x, w, bias, H.ACT[act])
        assert np.isnan(ref[2]).all() and np.isinf(ref[0]).all() == (act == "NONE") and np.isfinite(ref[3]).all()
        H.check(run_fc(gpu_lib, x, w, bias, act), ref, tol, "non-finite fc_f32_kernel " + act)


def test_nonfinite_eltwise(gpu_lib):
    rng = np.random.default_rng(703)
    a, b = plant(act_input(rng, FULL)), plant(weights(rng, (1, 5, 7, 6)))[:, ::-1].copy()
    for kind in ("add", "sub", "mul", "sqdiff"):
        for act in NONFINITE_ACTS:
            ref, tol = H.eltwise_ref(a, b, kind, H.ACT[act])
            assert np.isnan(ref).any()
            H.check(run_eltwise(gpu_lib, a, b, kind, act), ref, tol,
                    "non-finite eltwise_f32_kernel %s %s" % (kind, act))


def test_nonfinite_pool(gpu_lib):
    rng = np.random.default_rng(704)
    x = plant(act_input(rng, (2, 8, 8, 3)))
    g = H.Geom((8, 8), (2, 2), 2, 1, False)
    for kind in ("avg", "max"):
        for act in NONFINITE_ACTS:
            ref, tol = H.pool_ref(x, kind, g, H.ACT[act])
            assert np.isnan(ref).any() == (kind == "avg")  # a maximum skips NaN, as std::max(acc, v) does
            H.check(run_pool(gpu_lib, x, kind, g, act), ref, tol, "non-finite pool_f32_kernel %s %s" % (kind, act))


def test_nonfinite_unary(gpu_lib):
    x = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, 0.5, 7.0, -np.nan] * 30, f32)
    for name in ("RELU", "RELU6", "RELU_N1_TO_1"):
        lo, hi = H.ACT[name]
        H.check(run_unary(gpu_lib, "clamp", x, lo, hi), *H.clamp_ref(x, lo, hi), "non-finite clamp " + name)
    H.check(run_unary(gpu_lib, "logistic", x), *H.logistic_ref(x), "non-finite logistic")
    ref, tol = H.rsqrt_ref(x)
    assert np.isnan(ref[3]) and np.isneginf(ref[4]) and ref[1] == 0  # RSQRT of a negative value is NaN
    H.check(run_unary(gpu_lib, "rsqrt", x), ref, tol, "non-finite rsqrt")


def test_nonfinite_softmax(gpu_lib):
    rng = np.random.default_rng(706)
    x = act_input(rng, (5, 70))
    x[0, 5], x[1, 69], x[2, 64] = np.nan, np.inf, -np.inf  # rows 3, 4 stay finite
    ref, tol = H.softmax_ref(x, f32(0.8))
    assert np.isnan(ref[0]).all() and np.isnan(ref[1]).all() and ref[2, 64] == 0 and np.isfinite(ref[2:]).all()
    H.check(run_softmax(gpu_lib, x, 0.8), ref, tol, "non-finite softmax_f32_kernel")


# ---- the float graphs op by op on the GPU worker ---------------------------
GRAPHS = {"float_zoo": float_zoo, "float_edge_zoo": float_edge_zoo}


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_every_op_gpu_worker(gpu_lib, name):
    from band_amd import DeviceFlag
    worst = check_all_ops(GRAPHS[name](), DeviceFlag.kGPU, 1, graph_feed, name + " kGPU")
    assert worst and max(worst.values()) <= 1.0


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_outputs_only_gpu_worker(gpu_lib, name):
    from band_amd import DeviceFlag
    check_outputs_only(GRAPHS[name](), DeviceFlag.kGPU, 1, name + " kGPU")


def test_nonfinite_gpu_worker(gpu_lib):
    from band_amd import DeviceFlag
    assert check_all_ops(float_zoo(), DeviceFlag.kGPU, 1, nonfinite_feed, "float_zoo kGPU non-finite")
