"""Directed parity of the int8 / uint8 launchers: chosen accumulators through
every conv / depthwise / FC epilogue form (tests/directed_harness.py),
saturating contractions, every byte pair through ADD / SUB / MUL and the fused
residual ADD, pooling of extreme planes.  Bit-exact against the oracle; every
forced or routed form is confirmed by name before it is launched.
"""
import ctypes

import numpy as np
import pytest

from oracle import runner as orc
from tests import directed_harness as dh
from tests.kernel_harness import ConvCase, dom

pytestmark = pytest.mark.gpu

I8, U8 = np.int8, np.uint8
FAMILIES = [("fast", I8), ("fast", U8), ("two", I8), ("two", U8)]


def launch(lib, c, name, what=""):
    """one directed / explicit ConvCase: the kernel by name, fast_ok as the
    family says, then bit-exact with requant_fast as chosen and forced off"""
    from band_amd import _abi
    ref = c.oracle()
    family = getattr(getattr(c, "epi", None), "family", None)
    seen = set()
    for fast in (None, False):
        c.requant_fast = fast
        keep = []
        p = c.params(lib, keep, expect=ref)
        namer = lib.bh_dwconv2d_i8_kernel if c.depthwise else lib.bh_conv2d_i8_kernel
        got_name = namer(ctypes.byref(p)).decode()
        assert got_name == name, "%s: routed to %s, wanted %s" % (what, got_name, name)
        if family is not None and fast is None:
            assert p.requant_fast == (1 if family == "fast" else 0), "%s: fast_ok %d" % (what, p.requant_fast)
        if p.requant_fast in seen:
            continue  # a two-step layer: forcing it off is the same launch
        seen.add(p.requant_fast)
        fn = lib.bh_dwconv2d_i8 if c.depthwise else lib.bh_conv2d_i8
        _abi.check(fn(ctypes.byref(p), None), name)
        got = c._dy.download(c.dtype, ref.shape)
        del keep
        np.testing.assert_array_equal(got, ref, err_msg="%s %s requant_fast %d" % (what, name, p.requant_fast))
    return ref


# --- 2. conv epilogues ------------------------------------------------------------

@pytest.mark.parametrize("family,dtype", FAMILIES)
def test_conv1x1_directed(gpu_lib, family, dtype):
    """K = 16, N = 256 (and the 32 channels of the e_max layer): conv_mfma /
    conv_gemm / conv_gemm_big forced at M = 256, conv_xs routed at M = 2304"""
    for i, epi in enumerate(dh.epilogues(family, dtype, 16)):
        if dtype == I8:
            forms = [(1, 1, "conv_mfma_kernel"), (2, 1, "conv_gemm_kernel"), (3, 1, "conv_gemm_big_kernel"),
                     (0, 9, "conv_xs_kernel")]
            w_zp = 0
        else:  # filter zero point at both ends: the swept byte is 1 / 254
            forms = [(1, 1, "conv_mfma_kernel"), (0, 9, "conv_xs_kernel")]
            w_zp = (0, 255)[i % 2]
        for hint, sweeps, name in forms:
            c = dh.conv_layer(epi, sweeps=sweeps, w_zp=w_zp, kernel_hint=hint, seed=i)
            launch(gpu_lib, c, name, epi.name)


@pytest.mark.parametrize("k", [4, 8, 20])
@pytest.mark.parametrize("family,dtype", FAMILIES)
def test_conv_xs_vector_widths_directed(gpu_lib, family, dtype, k):
    """conv_xs_kernel's 4- / 8-byte K vectors (K = 16 above is the 16-byte one)"""
    for i, epi in enumerate(dh.epilogues(family, dtype, k)):
        w_zp = 0 if dtype == I8 else (255, 0)[i % 2]
        launch(gpu_lib, dh.conv_layer(epi, ic=k, sweeps=9, w_zp=w_zp, seed=i), "conv_xs_kernel", epi.name)


@pytest.mark.parametrize("family,dtype", FAMILIES)
def test_conv_direct_directed(gpu_lib, family, dtype):
    """3x3, in_c = 4, SAME: the sweep sits under the centre tap; the taps that
    fall outside the image contribute nothing, as in TFLite"""
    for i, epi in enumerate(dh.epilogues(family, dtype, 36)):
        w_zp = 0 if dtype == I8 else (0, 255)[i % 2]
        launch(gpu_lib, dh.conv_layer(epi, ic=4, k=3, w_zp=w_zp, seed=i), "conv_direct_kernel", epi.name)


STEM_FORMS = {0: "conv_stem_mfma_kernel", 4: "conv_stem_lds_kernel", 5: "conv_stem_mfma_kernel",
              6: "conv_stem_kernel"}


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("family,dtype", FAMILIES)
def test_conv_stem_directed(gpu_lib, family, dtype, stride):
    """the four stem forms (routed = MFMA, LDS-staged VALU, MFMA forced,
    scalar-cache VALU) on in_c = 3, 64 channels per layer"""
    for i, epi in enumerate(dh.epilogues(family, dtype, 27)):
        w_zp = 0 if dtype == I8 else (0, 255)[i % 2]
        for j, part in enumerate(dh.chunks(epi, 64, multiple=16)):
            for hint, name in STEM_FORMS.items():
                c = dh.conv_layer(part, ic=3, k=3, stride=stride, w_zp=w_zp, kernel_hint=hint, seed=i)
                launch(gpu_lib, c, name, "%s part %d hint %d" % (epi.name, j, hint))


@pytest.mark.parametrize("family", ["fast", "two"])
def test_conv_group_directed(gpu_lib, family):
    """bh_conv_group_i8 with a deep (K = 192: split-K form) and a shallow
    (K = 16) directed member"""
    from band_amd import _abi
    from band_amd.device import DeviceBuffer
    deep, shallow = dh.epilogues(family, I8, 192), dh.epilogues(family, I8, 16)
    for i in range(len(shallow)):
        convs = [dh.conv_layer(deep[i % len(deep)], ic=192, seed=i), dh.conv_layer(shallow[i], seed=i)]
        refs = [cc.oracle() for cc in convs]
        for fast in (None, False):
            keep, params = [], []
            for cc, ref in zip(convs, refs):
                cc.requant_fast = fast
                params.append(cc.params(gpu_lib, keep, expect=ref))
                cc._dy_keep = cc._dy
                assert gpu_lib.bh_conv_group_ok(ctypes.byref(params[-1])) == 1
                if fast is None:
                    assert params[-1].requant_fast == (1 if family == "fast" else 0)
            arr = (_abi.ConvParams * 2)(*params)
            host = np.zeros(gpu_lib.bh_conv_group_table_bytes(2), np.uint8)
            g = _abi.ConvGroup()
            _abi.check(gpu_lib.bh_conv_group_plan(arr, 2, host.ctypes.data_as(ctypes.c_void_p), ctypes.byref(g)), "plan")
            dt = DeviceBuffer.from_array(host)
            g.table = dt.value
            _abi.check(gpu_lib.bh_conv_group_i8(ctypes.byref(g), None), "bh_conv_group_i8")
            for j, cc in enumerate(convs):
                got = cc._dy_keep.download(cc.dtype, (cc.b, cc.oh, cc.ow, cc.oc))
                np.testing.assert_array_equal(got, refs[j], err_msg="%s member %d fast %s" % (cc.epi.name, j, fast))
            del keep, dt
            if family == "two":
                break


# --- 2. depthwise epilogues ---------------------------------------------------------

@pytest.mark.parametrize("family,dtype", FAMILIES)
def test_dwconv_directed(gpu_lib, family, dtype):
    """centre tap w_zp +- 1, every channel swept by its own byte plane: the
    run / dot / MFMA forms forced, the per-tap kernel (no tap table), dilation 2"""
    for i, epi in enumerate(dh.epilogues(family, dtype, 9)):
        w_zp = 0 if dtype == I8 else (1, 254)[i % 2]
        for hint, name in ((1, "dwconv3x3_run_kernel"), (2, "dwconv3x3_dot_kernel"), (3, "dwconv3x3_mfma_kernel")):
            launch(gpu_lib, dh.dw_layer(epi, w_zp=w_zp, kernel_hint=hint, seed=i), name, epi.name)
        launch(gpu_lib, dh.dw_layer(epi, w_zp=w_zp, taps=False, seed=i), "dwconv3x3_kernel", epi.name)
        for hint, name in ((1, "dwconv3x3_run_kernel"), (2, "dwconv3x3_dot_kernel")):
            launch(gpu_lib, dh.dw_layer(epi, w_zp=w_zp, dil=2, kernel_hint=hint, seed=i), name, epi.name + " dil 2")


@pytest.mark.parametrize("family,dtype", FAMILIES)
def test_dwconv_generic_directed(gpu_lib, family, dtype):
    """dwconv_generic_kernel: depth multiplier 2 (two output channels per swept
    plane) and a 5x5 window"""
    for i, epi in enumerate(dh.epilogues(family, dtype, 9)):
        w_zp = 0 if dtype == I8 else (254, 1)[i % 2]
        launch(gpu_lib, dh.dw_layer(epi, dm=2, w_zp=w_zp, seed=i), "dwconv_generic_kernel", epi.name + " dm 2")
    for i, epi in enumerate(dh.epilogues(family, dtype, 25)):
        w_zp = 0 if dtype == I8 else (1, 254)[i % 2]
        launch(gpu_lib, dh.dw_layer(epi, k=5, w_zp=w_zp, seed=i), "dwconv_generic_kernel", epi.name + " 5x5")


# --- 2. FC ------------------------------------------------------------------------------

def run_fc(lib, x, w, bias, *, in_zp, w_zp, out_zp, mult, shift, amin, amax, table=None):
    """bh_fc_i8 with per-unit multipliers on the executor's host packing; the
    oracle's FULLY_CONNECTED (-> table) is the reference"""
    from band_amd import _abi
    from band_amd.device import DeviceBuffer
    dtype = x.dtype
    rows, depth = x.shape
    units = w.shape[0]
    ref = orc.fully_connected(x, w, bias, in_zp=in_zp, w_zp=w_zp, out_zp=out_zp, mult=mult, shift=shift,
                              amin=amin, amax=amax)
    depth_pad = (depth + 15) // 16 * 16
    wd = w.astype(np.int32) - (0 if dtype == I8 else 128)
    in_zd, w_zd = dom(in_zp, dtype), dom(w_zp, dtype) if dtype == U8 else 0
    packed = np.zeros((units, depth_pad), np.int8)
    packed[:, :depth] = wd.astype(np.int8)
    beff = (bias.astype(np.int64) - in_zd * wd.sum(1) + depth * in_zd * w_zd).astype(np.int32)
    dx, dy = DeviceBuffer.from_array(x), DeviceBuffer(ref.nbytes)
    dw, db = DeviceBuffer.from_array(packed), DeviceBuffer.from_array(beff)
    dm = DeviceBuffer.from_array(np.ascontiguousarray(mult, np.int32))
    ds = DeviceBuffer.from_array(np.ascontiguousarray(shift, np.int32))
    p = _abi.FcParams(rows=rows, depth=depth, depth_pad=depth_pad, units=units,
                      in_xor=0 if dtype == I8 else 0x80, in_zp=in_zd, w_zp=w_zd, out_zp=out_zp,
                      act_min=amin, act_max=amax, input=dx.value, output=dy.value, weights=dw.value,
                      bias_eff=db.value, mult=dm.value, shift=ds.value)
    if table is not None:
        dt = DeviceBuffer.from_array(table)
        p.out_table = dt.value
        ref = table[ref.view(U8)].view(dtype)
    _abi.check(lib.bh_fc_i8(ctypes.byref(p), None), "fc")
    return dy.download(dtype, ref.shape), ref


@pytest.mark.parametrize("dtype,w_zp", [(I8, 0), (U8, 1), (U8, 254)])
@pytest.mark.parametrize("depth", [16, 37])
def test_fc_directed(gpu_lib, dtype, w_zp, depth):
    """FC has only the two-step form: the two-step triples, one unit each, 256
    rows, once more through a permutation out_table"""
    table = np.random.default_rng(77).permutation(256).astype(U8)
    for i, epi in enumerate(dh.epilogues("two", dtype, 16)):
        x, w, bias, _ = dh.fc_layer(epi, depth, w_zp, seed=i)
        kw = dict(in_zp=epi.in_zp, w_zp=w_zp, out_zp=epi.out_zp, mult=epi.mult, shift=epi.shift,
                  amin=epi.amin, amax=epi.amax)
        got, ref = run_fc(gpu_lib, x, w, bias, **kw)
        np.testing.assert_array_equal(got, ref, err_msg=epi.name)
        if i == 0:
            got, ref = run_fc(gpu_lib, x, w, bias, table=table, **kw)
            np.testing.assert_array_equal(got, ref, err_msg=epi.name + " table")


# --- 3. saturating contractions ---------------------------------------------------------

def extreme_planes(dtype, b, h, w, ic, pattern):
    lo, hi = dh.type_range(dtype)
    if pattern == "lo":
        return np.full((b, h, w, ic), lo, dtype)
    if pattern == "hi":
        return np.full((b, h, w, ic), hi, dtype)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    board = np.where((yy + xx) % 2 == 0, lo, hi)
    return np.broadcast_to(board[None, :, :, None], (b, h, w, ic)).astype(dtype)


def saturating_case(dtype, b, hw, ic, oc, k, pattern, in_end, w_end, depthwise=False, **kw):
    """all-extreme activations and filters: channel c has its first taps at one
    extreme and the rest at the other, the split moving with c, so |acc| runs
    from 0 up to K * 255 * 255 (uint8; K * 255 * 127 for int8) across the
    channels; each channel has its own bias and multiplier, sized so that the
    outputs spread over the window"""
    rng = np.random.default_rng(8000 + ic + oc + k + hw)
    lo, hi = dh.type_range(dtype)
    wlo, whi = (-127, 127) if dtype == I8 else (0, 255)
    in_zp = (lo, hi)[in_end]
    w_zp = 0 if dtype == I8 else (0, 255)[w_end]
    c = ConvCase(rng, b, hw, hw, ic, oc, k, k, dtype=dtype, act=0, depthwise=depthwise, **kw)
    oc = c.oc
    K = k * k * (1 if depthwise else ic)
    split = np.round(np.linspace(0, K, oc)).astype(int)
    taps = np.where(np.arange(K)[None, :] < split[:, None], whi, wlo)  # (oc, K)
    if depthwise:
        c.w = np.ascontiguousarray(taps.T.reshape(1, k, k, oc)).astype(dtype)
    else:
        c.w = taps.reshape(oc, k, k, ic).astype(dtype)
    c.w_zp, c.in_zp = w_zp, in_zp
    c.x = extreme_planes(dtype, b, hw, hw, ic, pattern)
    amax_acc = K * 255 * (127 if dtype == I8 else 255)
    c.bias = rng.integers(-amax_acc // 8, amax_acc // 8 + 1, oc).astype(np.int32)
    # real multiplier 100 / max|acc| times 1 / 2, 1 or 2: QuantizeMultiplier's
    # own output, so the parameters are ones TFLite would produce
    ms = [orc.quantize_multiplier(100.0 / amax_acc * f) for f in (0.5, 1.0, 2.0)]
    c.mult = np.array([ms[j % 3][0] for j in range(oc)], np.int32)
    c.shift = np.array([ms[j % 3][1] for j in range(oc)], np.int32)
    c.out_zp = 0 if dtype == I8 else 128
    c.amin, c.amax = lo, hi
    return c


def check_spread(ref, c, what):
    inside = int(((ref.astype(np.int64) > c.amin) & (ref.astype(np.int64) < c.amax)).sum())
    assert inside >= 0.25 * ref.size, "%s: %d of %d outputs inside the window" % (what, inside, ref.size)


@pytest.mark.parametrize("pattern", ["lo", "hi", "board"])
@pytest.mark.parametrize("dtype,ends", [(I8, (0, 0)), (I8, (1, 0)), (U8, (0, 1)), (U8, (1, 0)), (U8, (0, 0)),
                                        (U8, (1, 1))])
def test_conv_saturating(gpu_lib, dtype, ends, pattern):
    """deep 1x1 (K = 1280, 1296) on 8x8, batch 2, through the routed form and
    each forced one, and a 3x3 with in_c = 144 on 4x4"""
    for ic in (1280, 1296):
        c = saturating_case(dtype, 2, 8, ic, 64, 1, pattern, *ends)
        ref = c.oracle()
        check_spread(ref, c, "1x1 K %d" % ic)
        keep = []
        routed = gpu_lib.bh_conv2d_i8_kernel(ctypes.byref(c.params(gpu_lib, keep))).decode()
        del keep
        forms = [(0, routed), (1, "conv_mfma_kernel")]
        if dtype == I8:
            forms += [(2, "conv_gemm_kernel"), (3, "conv_gemm_big_kernel")]
        for hint, name in forms:
            c.kernel_hint = hint
            launch(gpu_lib, c, name, "saturating 1x1 K %d %s" % (ic, pattern))
    c = saturating_case(dtype, 2, 4, 144, 48, 3, pattern, *ends)
    check_spread(c.oracle(), c, "3x3")
    launch(gpu_lib, c, "conv_mfma_kernel", "saturating 3x3 %s" % pattern)


@pytest.mark.parametrize("pattern", ["lo", "hi", "board"])
@pytest.mark.parametrize("dtype,ends", [(I8, (0, 0)), (I8, (1, 0)), (U8, (0, 1)), (U8, (1, 0))])
def test_dwconv_saturating(gpu_lib, dtype, ends, pattern):
    for hint, taps, name in ((1, True, "dwconv3x3_run_kernel"), (2, True, "dwconv3x3_dot_kernel"),
                             (3, True, "dwconv3x3_mfma_kernel"), (0, False, "dwconv3x3_kernel")):
        c = saturating_case(dtype, 2, 8, 32, 0, 3, pattern, *ends, depthwise=True, kernel_hint=hint, taps=taps)
        check_spread(c.oracle(), c, "depthwise")
        launch(gpu_lib, c, name, "saturating depthwise %s" % pattern)


@pytest.mark.parametrize("pattern", ["lo", "hi"])
@pytest.mark.parametrize("dtype,ends", [(I8, (0, 0)), (I8, (1, 0)), (U8, (0, 1)), (U8, (1, 0))])
def test_fc_saturating(gpu_lib, dtype, ends, pattern):
    c = saturating_case(dtype, 2, 1, 1280, 64, 1, pattern, *ends)
    got, ref = run_fc(gpu_lib, c.x.reshape(2, 1280), c.w.reshape(64, 1280), c.bias, in_zp=c.in_zp, w_zp=c.w_zp,
                      out_zp=c.out_zp, mult=c.mult, shift=c.shift, amin=c.amin, amax=c.amax)
    check_spread(ref, c, "fc")
    np.testing.assert_array_equal(got, ref)


# --- 4. ADD / SUB / MUL on every byte pair ----------------------------------------------

def eltwise_sets(dtype):
    """(kind, sub, scales, zero points, activation): parameter sets that come
    out of TFLite's own Prepare (orc.add_params / orc.mul_params)"""
    z = (lambda *v: v) if dtype == I8 else (lambda *v: tuple(x + 128 for x in v))
    out = []
    # ADD / SUB: s1 / s2 of 1, 1 / 256, 300, 500; zero points at both ends and
    # in the middle; the four activation windows
    for (sa, sb, so), zps, act, sub in [
            ((0.02, 0.02, 0.04), z(-128, 127, 0), 0, False),
            ((0.02, 0.02, 0.04), z(-128, 127, -128), 1, True),
            ((6 / 255, 6 / 255, 6 / 255), z(-128, -128, -128), 3, False),
            ((0.01, 0.01, 1 / 127), z(0, 0, 0), 2, False),
            ((0.0001, 0.0256, 0.03), z(-128, 127, 5), 0, False),
            ((0.0001, 0.0256, 0.0256), z(127, 0, 127), 0, True),
            ((0.03, 0.0001, 0.03), z(0, -128, -128), 1, False),
            ((0.01, 0.01 / 300, 1 / 127), z(3, 127, 0), 2, True),
            ((0.05, 0.0001, 0.05), z(-128, 127, 0), 0, False),
            ((6 / 255, 6 / 255 / 500, 6 / 255), z(-128, 0, -128), 3, False)]:
        out.append(("add", sub, (sa, sb, so), zps, act))
    # MUL: negative shifts at the same zero points, then two left shifts
    for (sa, sb, so), zps, act in [
            ((0.02, 0.02, 0.02 * 0.02 * 260), z(-128, -128, -128), 0),
            ((0.02, 0.02, 0.02 * 0.02 * 130), z(0, 0, 0), 0),
            ((0.02, 0.03, 0.02 * 0.03 * 260), z(127, 127, -128), 1),
            ((6 / 255, 6 / 255, 6 / 255), z(-128, -128, -128), 3),
            ((0.01, 0.01, 1 / 127), z(127, -128, 0), 2),
            ((0.1, 0.1, 0.009), z(0, 0, 0), 0),
            ((0.05, 0.05, 0.0007), z(3, -5, 10), 0)]:
        out.append(("mul", False, (sa, sb, so), zps, act))
    return out


def eltwise_ref(kind, sub, scales, zps, act, a, b):
    dtype = a.dtype
    sa, sb, so = scales
    za, zb, zo = zps
    amin, amax = orc.act_range(act, so, zo, dtype == I8)
    if kind == "add":
        prm = orc.add_params(sa, sb, so)
        ref = orc.add(a, b, a_zp=za, b_zp=zb, out_zp=zo, params=prm, amin=amin, amax=amax, sub=sub)
    else:
        prm = orc.mul_params(sa, sb, so)
        ref = orc.mul(a, b, a_zp=za, b_zp=zb, out_zp=zo, mult=prm[0], shift=prm[1], amin=amin, amax=amax)
    return ref, prm, amin, amax


def run_eltwise(lib, kind, sub, zps, prm, amin, amax, a, b, out_shape):
    from band_amd import _abi
    from band_amd.device import DeviceBuffer
    s4 = lambda s: [1] * (4 - len(s)) + list(s)
    p = _abi.EltwiseParams()
    p.kind = 0 if kind == "add" else 1
    p.in_signed = int(a.dtype == I8)
    for i, (x, y, z) in enumerate(zip(s4(a.shape), s4(b.shape), s4(out_shape))):
        p.shape_a[i], p.shape_b[i], p.shape_o[i] = x, y, z
    p.a_off, p.b_off, p.o_off = -zps[0], -zps[1], zps[2]
    if kind == "add":
        p.a_mult, p.a_shift, p.b_mult, p.b_shift, p.o_mult, p.o_shift, p.left_shift = [int(v) for v in prm]
        if sub:
            p.b_mult = -p.b_mult
    else:
        p.o_mult, p.o_shift = prm
    p.act_min, p.act_max = amin, amax
    da, db = DeviceBuffer.from_array(a), DeviceBuffer.from_array(b)
    do = DeviceBuffer(int(np.prod(out_shape)))
    p.a, p.b, p.out = da.value, db.value, do.value
    _abi.check(lib.bh_eltwise_i8(ctypes.byref(p), None), "eltwise")
    return do.download(a.dtype, out_shape)


@pytest.mark.parametrize("dtype", [I8, U8])
def test_eltwise_every_byte_pair(gpu_lib, dtype):
    """all 65,536 (a, b) pairs through eltwise_flat4_kernel (equal shapes) and
    eltwise_bcast_kernel (a column against a row; a one-element operand)"""
    lo, _ = dh.type_range(dtype)
    col = (np.arange(256) + lo).astype(dtype).reshape(1, 256, 1, 1)
    row = (np.arange(256) + lo).astype(dtype).reshape(1, 1, 256, 1)
    fa = np.ascontiguousarray(np.broadcast_to(col, (1, 256, 256, 1)))
    fb = np.ascontiguousarray(np.broadcast_to(row, (1, 256, 256, 1)))
    left_shifts = 0
    for kind, sub, scales, zps, act in eltwise_sets(dtype):
        what = "%s sub %s scales %r zps %r act %d" % (kind, sub, scales, zps, act)
        ref, prm, amin, amax = eltwise_ref(kind, sub, scales, zps, act, fa, fb)
        inside = int(((ref.astype(np.int64) > amin) & (ref.astype(np.int64) < amax)).sum())
        if kind == "mul" and prm[1] > 0:
            left_shifts += 1
            distinct = len(np.unique(ref))
            assert inside >= 1000 and distinct >= 64, "%s: %d inside, %d distinct" % (what, inside, distinct)
        else:
            assert inside >= 16384, "%s: %d pairs inside the window" % (what, inside)
        got = run_eltwise(gpu_lib, kind, sub, zps, prm, amin, amax, fa, fb, ref.shape)
        np.testing.assert_array_equal(got, ref, err_msg="flat4 " + what)
        got = run_eltwise(gpu_lib, kind, sub, zps, prm, amin, amax, col, row, ref.shape)
        np.testing.assert_array_equal(got, ref, err_msg="bcast " + what)
        for v in (0, 128, 255):  # a one-element second operand
            one = row.reshape(-1)[v:v + 1]
            got = run_eltwise(gpu_lib, kind, sub, zps, prm, amin, amax, fa, one, ref.shape)
            np.testing.assert_array_equal(got, ref[:, :, v:v + 1, :] + np.zeros_like(ref), err_msg="(1,) " + what)
    assert left_shifts >= 2


# --- 5. fused residual ADD + output table on every (y, r) pair --------------------------

def passthrough_epi(dtype=I8, k=16):
    """256 channels of (2^31 - 1, shift 0, sweep -128 .. 127), output zero point
    0, full window: y takes all 256 values over the 256 pixels of a sweep"""
    n = 256
    lo, hi = dh.type_range(dtype)
    return dh.Epi("passthrough", "fast", dtype, k, np.full(n, (1 << 31) - 1, np.int64), np.zeros(n, np.int64),
                  np.full(n, -128, np.int64), 0 if dtype == I8 else 128, lo, hi, -128 if dtype == I8 else 0)


RESIDUAL_SETS = [  # (y scale, residual scale, out scale), (y_zp is the conv's, r_zp, o_zp), activation
    ((0.05, 0.05 / 64, 0.05), (127, -128), 0), ((0.05, 0.05, 0.1), (127, 127), 0),
    ((0.05 / 64, 0.05, 0.05), (0, 0), 1), ((0.02, 0.02, 0.03), (-128, -128), 0)]


def run_residual(lib, c, name, what=""):
    """conv -> ADD -> table against the oracle's three ops, every (y, r) pair:
    residual[pixel, c] = the c-th value of the layer's type, with and without
    a permutation out_table, both requantisation paths.  A uint8 layer takes
    the sets' zero points moved by 128, its residual read unsigned."""
    from band_amd import _abi
    from band_amd.device import DeviceBuffer
    dtype = np.dtype(c.dtype)
    lo = dh.type_range(dtype)[0]
    y = c.oracle()
    assert y.dtype == dtype
    assert all(len(np.unique(y[0, :, :, ch])) == 256 for ch in (0, 1, 255)), "y does not sweep"
    r = np.ascontiguousarray(np.broadcast_to((np.arange(256) + lo).astype(dtype), y.shape))
    table = np.random.default_rng(5).permutation(256).astype(U8)
    for (ys, rs, os_), zps, act in RESIDUAL_SETS:
        r_zp, o_zp = (z + lo + 128 for z in zps)
        prm = orc.add_params(ys, rs, os_)
        amin, amax = orc.act_range(act, os_, o_zp, dtype == I8)
        z = orc.add(y, r, a_zp=c.out_zp, b_zp=r_zp, out_zp=o_zp, params=prm, amin=amin, amax=amax)
        for with_table in (False, True):
            ref = table[z.view(U8)].view(dtype) if with_table else z
            for fast in (None, False):
                c.requant_fast = fast
                keep = []
                p = c.params(lib, keep, expect=ref)
                dr = DeviceBuffer.from_array(r)
                keep.append(dr)
                p.residual = dr.value
                if with_table:
                    dt = DeviceBuffer.from_array(table)
                    keep.append(dt)
                    p.out_table = dt.value
                p.add_left_shift = int(prm[6])
                p.add_y_off, p.add_r_off, p.add_o_off = -c.out_zp, -r_zp, o_zp
                p.add_y_mult, p.add_y_shift = int(prm[0]), int(prm[1])
                p.add_r_mult, p.add_r_shift = int(prm[2]), int(prm[3])
                p.add_o_mult, p.add_o_shift = int(prm[4]), int(prm[5])
                p.add_act_min, p.add_act_max = amin, amax
                got_name = lib.bh_conv2d_i8_kernel(ctypes.byref(p)).decode()
                assert got_name == name, "%s: routed to %s, wanted %s" % (what, got_name, name)
                assert p.requant_fast == (1 if fast is None else 0)
                _abi.check(lib.bh_conv2d_i8(ctypes.byref(p), None), "bh_conv2d_i8")
                got = c._dy.download(dtype, y.shape)
                del keep
                np.testing.assert_array_equal(got, ref, err_msg="%s %s scales %r table %s fast %s" % (
                    what, name, (ys, rs, os_), with_table, fast))


@pytest.mark.parametrize("hint,sweeps,k,ic,name", [
    (1, 1, 1, 16, "conv_mfma_kernel"), (3, 1, 1, 16, "conv_gemm_big_kernel"), (0, 9, 1, 16, "conv_xs_kernel"),
    (0, 1, 3, 4, "conv_direct_kernel")])
def test_conv_residual_every_pair(gpu_lib, hint, sweeps, k, ic, name):
    c = dh.conv_layer(passthrough_epi(k=k * k * ic), ic=ic, k=k, sweeps=sweeps, kernel_hint=hint)
    run_residual(gpu_lib, c, name)


@pytest.mark.parametrize("hint,sweeps,k,ic,name", [
    (1, 1, 1, 16, "conv_mfma_kernel"), (0, 9, 1, 16, "conv_xs_kernel"), (7, 1, 1, 16, "conv_rows_kernel"),
    (0, 1, 3, 4, "conv_direct_kernel")])
def test_conv_residual_every_pair_uint8(gpu_lib, hint, sweeps, k, ic, name):
    """the unsigned branch of the folded ADD (in_xor != 0: conv_store4, conv_xs,
    conv_rows, conv_direct): y and the residual as uint8, same layer.
    conv_gemm_big_kernel has no such run: its route admits int8 activations only."""
    c = dh.conv_layer(passthrough_epi(dtype=U8, k=k * k * ic), ic=ic, k=k, sweeps=sweeps, kernel_hint=hint)
    run_residual(gpu_lib, c, name)


# --- 7. conv_rows_kernel: reached by hint only (BH_CONV_ROWS = 7) ------------------------

def test_conv_rows_kernel(gpu_lib):
    """conv_rows_kernel by name on three of test_conv1x1_rows_batched's layers
    at reduced batch and a K > 320 one, the fast and two-step directed layers
    of both dtypes, the residual pairs and the saturating deep-K layers"""
    lib, name, hint = gpu_lib, "conv_rows_kernel", 7
    for b, spatial, ic, oc, dtype in [(2, 28, 32, 192, I8), (8, 14, 96, 20, U8), (40, 7, 64, 520, I8),
                                      (8, 7, 384, 520, I8), (8, 7, 328, 24, U8)]:
        rng = np.random.default_rng(4000 + b + spatial + ic + oc)
        launch(lib, ConvCase(rng, b, spatial, spatial, ic, oc, 1, 1, dtype=dtype, act=3, kernel_hint=hint), name,
               "rows %d" % ic)
    for family, dtype in FAMILIES:
        for i, epi in enumerate(dh.epilogues(family, dtype, 16)):
            w_zp = 0 if dtype == I8 else (0, 255)[i % 2]
            launch(lib, dh.conv_layer(epi, w_zp=w_zp, kernel_hint=hint, seed=i), name, epi.name)
    run_residual(lib, dh.conv_layer(passthrough_epi(), kernel_hint=hint), name)
    for dtype, ends in ((I8, (1, 0)), (U8, (0, 1)), (U8, (1, 0))):  # saturating, K = 1280 / 1296
        for ic in (1280, 1296):
            c = saturating_case(dtype, 2, 8, ic, 64, 1, "board", *ends, kernel_hint=hint)
            check_spread(c.oracle(), c, "rows saturating")
            launch(lib, c, name, "saturating K %d" % ic)


# --- 8. pooling of extreme planes under a narrow window ---------------------------------

@pytest.mark.parametrize("kind", ["avg", "max"])
@pytest.mark.parametrize("dtype", [I8, U8])
@pytest.mark.parametrize("shape,f,s,same", [
    ((1, 9, 9, 8), 3, 2, True),      # pool_kernel<4>, clipped SAME windows
    ((1, 9, 9, 5), 3, 2, True),      # pool_kernel<1>
    ((1, 7, 7, 64), 7, 1, False),    # pool_wide_kernel<4>
    ((1, 7, 7, 64), 7, 3, True),     # pool_wide_kernel<4>, clipped
    ((2, 14, 14, 16), 14, 1, False),  # pool_wide_kernel<16>
    ((2, 14, 14, 16), 14, 5, True),  # pool_wide_kernel<16>, clipped
])
def test_pool_extremes(gpu_lib, kind, dtype, shape, f, s, same):
    from band_amd import _abi
    from band_amd.device import DeviceBuffer
    b, ih, iw, ch = shape
    lo, hi = dh.type_range(dtype)
    oh, ow = orc.out_size(same, ih, f, s, 1), orc.out_size(same, iw, f, s, 1)
    ph, pw = orc.padding(s, 1, ih, f, oh), orc.padding(s, 1, iw, f, ow)
    mid = (lo + hi + 1) // 2
    # the type's window, one narrower at the low end, one around the middle
    # (where the checkerboard's averages land)
    for pattern in ("lo", "hi", "board"):
        x = extreme_planes(dtype, b, ih, iw, ch, pattern)
        for amin, amax in ((lo, hi), (lo, lo + 60), (mid - 30, mid + 30), (hi - 60, hi)):
            ref = orc.pool2d(x, kind=kind, filt=(f, f), stride=(s, s), pad=(ph, pw), out_hw=(oh, ow),
                             amin=amin, amax=amax)
            dx, dy = DeviceBuffer.from_array(x), DeviceBuffer(ref.nbytes)
            p = _abi.PoolParams(kind=0 if kind == "avg" else 1, in_signed=int(dtype == I8), batch=b, in_h=ih,
                                in_w=iw, channels=ch, out_h=oh, out_w=ow, f_h=f, f_w=f, stride_h=s, stride_w=s,
                                pad_h=ph, pad_w=pw, act_min=amin, act_max=amax, input=dx.value, output=dy.value)
            _abi.check(gpu_lib.bh_pool_i8(ctypes.byref(p), None), "pool")
            np.testing.assert_array_equal(dy.download(dtype, ref.shape), ref,
                                          err_msg="%s window [%d, %d]" % (pattern, amin, amax))
