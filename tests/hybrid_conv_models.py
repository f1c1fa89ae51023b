"""Fixtures of the dynamic-range ("hybrid") CONV_2D / DEPTHWISE_CONV_2D -
float32 input, constant int8 filter with zero points 0, each batch item
quantised at run time: the numpy restatement of the rule, its deliberately
wrong variants, the launcher cases, the models and the rule on one operator of
a graph (hybrid_conv_reference, for tests.float_harness.check_graph_ops).

The rule (DESIGN 4 holds it in words; restated from memory of TFLite's conv.cc
EvalHybrid / EvalHybridPerChannel, depthwise_conv.cc EvalHybridPerChannel and
the reference hybrid kernels, parity unpinned beyond that text).  Every float
operation is one IEEE float32 operation - an explicit .astype(np.float32) after
each; round is half away from zero.

  item b             the H W C floats of image b, quantised by the row rule of
                     tests.hybrid_models.np_dynquant with the item as the row:
                     q, s[b], off[b]
  acc                sum over the in-bounds taps of w (q - off[b])   (int32, exact)
  CONV_2D, 1 scale   symmetric items; y = bias[c] + (float)acc * (s[b] * ws)
  CONV_2D, out_c     asymmetric items; y = ((float)acc * ws[c]) * s[b] + bias[c]
  DEPTHWISE, out_c   asymmetric items; y = (float)acc * (ws[c] * s[b]) + bias[c]
  all                a missing bias adds 0; clamped to the fused activation

tests/test_conv_hybrid_cpu.py first judges this restatement alone: against the
float64 convolution of the dequantised filter at a derived bound, and against
its wrong variants."""
import ctypes
import math

import numpy as np

from band_amd.tflite_synth import FGraph, mobilenet_v1, mobilenet_v2, vit_tiny
from tests import float_harness as H
from tests import hybrid_models as Y

F = np.float32
F64 = np.float64
CONV_2D, DEPTHWISE_CONV_2D = 3, 4
DQ_ONE, DQ_TWO = "dynquant_item_kernel", "dynquant_minmax_kernel+dynquant_items_kernel"
CONV_KERNEL, DW_KERNEL = "conv_hybrid_kernel", "dwconv_hybrid_kernel"
ACTS = Y.ACTS
SLACK = Y.SLACK
NAN_WORD = Y.NAN_WORD
CHUNK = 4096             # BH_DYNQUANT_CHUNK
ONE_LAUNCH_MAX = 16384   # BH_DYNQUANT_ONE_LAUNCH_MAX
FORMS = ("pt", "pc", "dw")  # CONV_2D one scale, CONV_2D out_c scales, DEPTHWISE_CONV_2D


# ---- the rule ----------------------------------------------------------------------------
def np_dynquant_items(x, asymmetric, wrong=None):
    """(q int8 like x, s float32 [B], off int32 [B]) of float32 x [B, ...].
    wrong: "whole_batch" one quantisation for the batch, "per_row" one per row of the last axis
    (s and off of an item then those of its first row)"""
    x = np.asarray(x, F)
    B = x.shape[0]
    if wrong == "whole_batch":
        q, s, off = Y.np_dynquant(x.reshape(1, -1), asymmetric)
        return q.reshape(x.shape), np.repeat(s, B), np.repeat(off, B)
    if wrong == "per_row":
        q, s, off = Y.np_dynquant(x.reshape(-1, x.shape[-1]), asymmetric)
        per = s.size // B
        return q.reshape(x.shape), s[::per].copy(), off[::per].copy()
    q, s, off = Y.np_dynquant(x.reshape(B, -1), asymmetric)
    return q.reshape(x.shape), s, off


def taps(v, g, fill):
    """[B, OH, OW, KH, KW, C] of v [B, H, W, C]: tap (ky, kx) of every output pixel, an
    out-of-bounds tap holding fill[b]"""
    B, Hh, Ww, C = v.shape
    (OH, OW), (KH, KW), (sh, sw), (dh, dw), (ph, pw) = g.out_hw, g.k_hw, g.stride, g.dilation, g.pad
    bot = max(0, (OH - 1) * sh - ph + (KH - 1) * dh - (Hh - 1))
    rgt = max(0, (OW - 1) * sw - pw + (KW - 1) * dw - (Ww - 1))
    padded = np.empty((B, ph + Hh + bot, pw + Ww + rgt, C), v.dtype)
    padded[...] = np.asarray(fill, v.dtype).reshape(B, 1, 1, 1)
    padded[:, ph:ph + Hh, pw:pw + Ww] = v
    out = np.empty((B, OH, OW, KH, KW, C), v.dtype)
    for ky in range(KH):
        for kx in range(KW):
            out[:, :, :, ky, kx] = padded[:, ky * dh:ky * dh + (OH - 1) * sh + 1:sh, kx * dw:kx * dw + (OW - 1) * sw + 1:sw]
    return out


def in_bounds(shape_hw, g):
    """[OH, OW, KH, KW] float64: 1 where the tap lies inside the input"""
    ones = np.ones((1,) + tuple(shape_hw) + (1,), F64)
    return taps(ones, g, [0.0])[0, ..., 0]


def _sum_taps(cols, w, form, dm):
    """sum over the taps: cols [B, OH, OW, KH, KW, C] with w OHWI (conv) or [1, KH, KW, C dm] (depthwise)"""
    if form == "dw":
        return np.einsum("byxijc,ijc->byxc", np.repeat(cols, dm, axis=-1), w[0])
    return np.einsum("byxijc,oijc->byxo", cols, w)


def np_epilogue(acc, s, ws, bias, form, act="NONE", wrong=None):
    """acc int64 [B, OH, OW, out_c], s float32 [B], ws float32 [out_c].
    wrong: "swap" the conv's out_c-scales order exchanged with the depthwise one, "fma" the last
    multiply and the bias as one fused multiply-add, "ws0" ws[0] for every channel"""
    assert np.abs(acc).max(initial=0) < 2 ** 31
    accf = acc.astype(F)
    ws = np.asarray(ws, F)
    if wrong == "ws0":
        ws = np.full_like(ws, ws[0])
    sb = np.asarray(s, F).reshape(-1, 1, 1, 1)
    b = (np.zeros(accf.shape[-1], F) if bias is None else np.asarray(bias, F)).reshape(1, 1, 1, -1)
    order = form
    if wrong == "swap":
        order = {"pc": "dw", "dw": "pc", "pt": "pc"}[form]
    if order == "pc":
        t1 = (accf * ws).astype(F)
        if wrong == "fma":
            y = (t1.astype(F64) * sb.astype(F64) + b.astype(F64)).astype(F)
        else:
            y = ((t1 * sb).astype(F) + b).astype(F)
    else:  # "pt": bias + acc (s ws); "dw": acc (ws s) + bias - the same three float operations
        sc = (sb * ws).astype(F)
        if wrong == "fma":
            y = (accf.astype(F64) * sc.astype(F64) + b.astype(F64)).astype(F)
        else:
            y = ((accf * sc).astype(F) + b).astype(F)
    lo, hi = H.ACT[act]
    return np.minimum(np.maximum(y, F(lo)), F(hi)).astype(F)


def np_acc(q, off, w, g, form, dm=1, wrong=None):
    """the integer sum.  wrong: "pad_zero" a padded tap filled with the byte 0 instead of off[b]
    (the row sum over all taps still subtracted), "no_rowsum" the row-sum term dropped"""
    q64, w64 = q.astype(np.int64), np.asarray(w, np.int8).astype(np.int64)
    if wrong == "pad_zero":
        full = _sum_taps(taps(q64, g, np.zeros_like(off, np.int64)), w64, form, dm)
        rowsum = w64[0].sum(axis=(0, 1)) if form == "dw" else w64.sum(axis=(1, 2, 3))
        return full - off.astype(np.int64).reshape(-1, 1, 1, 1) * rowsum.reshape(1, 1, 1, -1)
    if wrong == "no_rowsum":
        return _sum_taps(taps(q64, g, off.astype(np.int64)), w64, form, dm)
    centred = taps(q64, g, off.astype(np.int64)) - off.astype(np.int64).reshape(-1, 1, 1, 1, 1, 1)
    return _sum_taps(centred, w64, form, dm)  # a padded tap holds off - off = 0


def np_conv_hybrid(x, w, ws, bias, g, form, act="NONE", dm=1, wrong=None):
    """float32 [B, OH, OW, out_c] of float32 x [B, H, W, C], int8 w, float32 ws [out_c]"""
    asym = form != "pt"
    q, s, off = np_dynquant_items(x, asym, wrong if wrong in ("whole_batch", "per_row") else None)
    acc = np_acc(q, off, w, g, form, dm, wrong if wrong in ("pad_zero", "no_rowsum") else None)
    return np_epilogue(acc, s, ws, bias, form, act, wrong if wrong in ("swap", "fma", "ws0") else None)


def real_conv(x, w, ws, bias, g, form, dm=1):
    """float64 convolution of x with the dequantised filter ws[c] w, plus bias"""
    y = _sum_taps(taps(np.asarray(x, F64), g, np.zeros(x.shape[0])), np.asarray(w, np.int8).astype(F64), form, dm)
    y = y * np.asarray(ws, F).astype(F64).reshape(1, 1, 1, -1)
    return y if bias is None else y + np.asarray(bias, F64).reshape(1, 1, 1, -1)


def quantisation_bound(x, w, ws, g, form, y, dm=1):
    """c s[b] ws[c] sum_in-bounds |w| + gamma(3) |y|: tests.hybrid_models.quantisation_bound with
    the sum over the taps that exist (c = 0.5 symmetric, 1 asymmetric)"""
    _, s, _ = np_dynquant_items(x, form != "pt")
    c = 0.5 if form == "pt" else 1.0
    absw = np.abs(np.asarray(w, np.int8).astype(F64))
    inb = in_bounds(x.shape[1:3], g)  # [OH, OW, KH, KW]
    if form == "dw":
        sums = np.einsum("yxij,ijc->yxc", inb, absw[0])
    else:
        sums = np.einsum("yxij,oijc->yxo", inb, absw)
    return (c * s.astype(F64).reshape(-1, 1, 1, 1) * np.asarray(ws, F).astype(F64).reshape(1, 1, 1, -1) * sums[None] +
            H.gamma(3) * np.abs(y))


# ---- launcher cases ----------------------------------------------------------------------
class DqCase:
    """items of `size` floats.  mode: "normal" (item b scaled by 1 + 0.7 b), "first" / "last" /
    "tail" (the extreme value at the first element, the last element, inside the last partial
    chunk), "pos", "neg", "zero", "const".  form: 1 one launch, 2 two launches, 0 the launcher's choice"""

    def __init__(self, size, batch, asymmetric, form, mode="normal", in_off=0, q_off=0, seed=0):
        rng = np.random.default_rng(3000 + seed + 13 * size + batch)
        self.size, self.batch, self.asymmetric, self.form, self.mode = size, batch, asymmetric, form, mode
        x = rng.normal(0, 1, (batch, size)).astype(F) * (1 + 0.7 * np.arange(batch, dtype=F))[:, None]
        if mode == "first":
            x[:, 0] = -37.5
        elif mode == "last":
            x[:, -1] = 41.25
        elif mode == "tail":
            x[:, size - max(1, (size % CHUNK) // 2)] = -52.0
        elif mode == "pos":
            x = np.abs(x) + F(0.25)
        elif mode == "neg":
            x = -np.abs(x) - F(0.25)
        elif mode == "zero":
            x[...] = 0
            if batch > 1:
                x[1:] = rng.normal(0, 1, (batch - 1, size))
        elif mode == "const":
            x[...] = F(0.7)
        self.x = x.astype(F)
        self.in_off, self.q_off = in_off, q_off
        self.name = "%dx%d_%s_f%d_%s%s" % (batch, size, "asym" if asymmetric else "sym", form, mode,
                                           "_off4" if in_off or q_off else "")

    def kernel(self):
        one = self.form == 1 or (self.form == 0 and self.size <= ONE_LAUNCH_MAX)
        return DQ_ONE if one else DQ_TWO

    def ref(self):
        return np_dynquant_items(self.x, self.asymmetric)


DQ_SIZES = (1, 3, 4, 63, 64, 65, 1023, 1024, 1025, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 1234)


def dq_cases():
    out = []
    for asym in (False, True):
        for form in (1, 2):
            for size in DQ_SIZES:
                out.append(DqCase(size, 3 if size % 2 else 1, asym, form, seed=size))
            out.append(DqCase(4096, 3, asym, form, seed=1))
            out.append(DqCase(65, 1, asym, form, seed=2))
            for mode in ("first", "last", "tail", "pos", "neg", "zero", "const"):
                out.append(DqCase(2 * CHUNK + 777, 3, asym, form, mode, seed=3))
                out.append(DqCase(2 * CHUNK + 776, 1, asym, form, mode, seed=4))  # float4 path
                out.append(DqCase(65, 3, asym, form, mode, seed=5))
            for size in (64, 1024, 2 * CHUNK + 776):
                out.append(DqCase(size, 3, asym, form, in_off=4, q_off=4, seed=6))
        # the launcher's own choice either side of the crossover
        out.append(DqCase(ONE_LAUNCH_MAX, 1, asym, 0, seed=7))
        out.append(DqCase(ONE_LAUNCH_MAX + 4, 3, asym, 0, "tail", seed=8))
    return out


class ConvCase:
    """x [batch, h, w, in_c] float32, item b scaled by 1 + 0.7 b (x_mode "pos" / "neg": all-positive
    / all-negative items, so that padding is off = -128 / 127); w uniform in +-127 (or w_fill);
    ws one scale ("pt") or out_c scales.  dm: depth multiplier ("dw": out_c = in_c dm)."""

    def __init__(self, form, batch, in_hw, in_c, out_c, k_hw, stride=1, dilation=1, same=True, bias=True, act="NONE",
                 seed=0, w_fill=None, x_mode="normal", in_off=0, q_off=0, out_off=0, dm=1, tag=""):
        assert form in FORMS
        pair = lambda v: (v, v) if np.isscalar(v) else tuple(v)  # noqa: E731
        k_hw, in_hw = pair(k_hw), pair(in_hw)
        if form == "dw":
            out_c = in_c * dm
        rng = np.random.default_rng(5000 + seed + 17 * in_c + 3 * out_c + in_hw[0] * in_hw[1] + k_hw[0])
        self.form, self.batch, self.in_hw, self.in_c, self.out_c, self.dm, self.act = form, batch, in_hw, in_c, out_c, dm, act
        self.g = H.Geom(in_hw, k_hw, stride, dilation, same)
        x = rng.normal(0, 1, (batch,) + in_hw + (in_c,)).astype(F)
        x *= (1 + 0.7 * np.arange(batch, dtype=F)).reshape(-1, 1, 1, 1)
        if x_mode == "pos":
            x = np.abs(x) + F(0.25)
        elif x_mode == "neg":
            x = -np.abs(x) - F(0.25)
        self.x = x.astype(F)
        wshape = (1,) + k_hw + (out_c,) if form == "dw" else (out_c,) + k_hw + (in_c,)
        self.w = (rng.integers(-127, 128, wshape) if w_fill is None else np.full(wshape, w_fill)).astype(np.int8)
        self.ws = (np.full(out_c, 0.0123, F) if form == "pt" else rng.uniform(0.004, 0.03, out_c).astype(F))
        self.bias = rng.normal(0, 1, out_c).astype(F) if bias else None
        self.in_off, self.q_off, self.out_off = in_off, q_off, out_off
        self.K = k_hw[0] * k_hw[1] * (1 if form == "dw" else in_c)
        self.M = batch * self.g.out_hw[0] * self.g.out_hw[1]
        self.name = "%s_b%d_%dx%dx%d_k%dx%d_s%s_d%s_%s_oc%d%s%s%s%s%s" % (
            form, batch, in_hw[0], in_hw[1], in_c, k_hw[0], k_hw[1], stride, dilation, "same" if same else "valid", out_c,
            "" if dm == 1 else "_dm%d" % dm, "" if bias else "_nobias", "" if act == "NONE" else "_" + act.lower(),
            "" if x_mode == "normal" else "_" + x_mode, tag)

    def quantised(self):
        return np_dynquant_items(self.x, self.form != "pt")

    def ref(self, wrong=None):
        return np_conv_hybrid(self.x, self.w, self.ws, self.bias, self.g, self.form, self.act, self.dm, wrong)


# (in_hw, in_c, k_hw): K = k_h k_w in_c over {1, 15, 16, 17, 27, 63, 64, 65, 130, 1280} with in_c in
# {1, 3, 4, 5, 16}, so that taps straddle the 16-byte fragments
K_SHAPES = (((3, 3), 1, (1, 1)), ((3, 5), 5, (1, 3)), ((3, 3), 16, (1, 1)), ((4, 4), 4, (2, 2)), ((1, 17), 1, (1, 17)),
            ((5, 5), 3, (3, 3)), ((3, 7), 3, (3, 7)), ((4, 4), 16, (2, 2)), ((2, 13), 5, (1, 13)), ((2, 13), 5, (2, 13)),
            ((16, 16), 5, (16, 16)), ((8, 10), 16, (8, 10)))
# (batch, in_hw) of 1 x 1 convs: M = 1, 15, 16, 17, 65
M_SHAPES = ((1, (1, 1)), (1, (3, 5)), (1, (4, 4)), (1, (1, 17)), (1, (5, 13)))
OUT_CS = (1, 15, 16, 17, 65)


def conv_cases():
    out, n = [], 0
    for form in ("pt", "pc"):
        def add(*a, **kw):
            nonlocal n
            n += 1
            kw.setdefault("seed", n)
            kw.setdefault("bias", n % 3 != 0)
            out.append(ConvCase(form, *a, **kw))
        for in_hw, in_c, k_hw in K_SHAPES:  # SAME: most of these pad
            add(1, in_hw, in_c, 17, k_hw)
            add(2, in_hw, in_c, 33, k_hw, same=False)
        for batch, in_hw in M_SHAPES:
            for oc in OUT_CS:
                add(batch, in_hw, 20, oc, 1)
        add(3, (3, 3), 8, 20, 3, tag="_tile_spans_items")           # out_h out_w = 9: a 16-row tile holds two items
        add(3, (3, 3), 8, 20, 3, x_mode="pos", tag="_tile_spans_items")
        for stride in (1, 2):
            add(2, (7, 6), 5, 19, 3, stride=stride)                  # SAME, the asymmetric pad at stride 2
            add(1, (8, 8), 16, 24, 3, stride=stride, x_mode="pos")
            add(1, (8, 8), 16, 24, 3, stride=stride, x_mode="neg")
        add(2, (9, 9), 4, 12, 3, same=False)
        add(2, (9, 8), 4, 12, 3, dilation=2)
        add(1, (9, 8), 3, 12, 3, dilation=2, same=False)
        add(2, (32, 32), 3, 48, 16, stride=16, same=False, tag="_patch")
        # the launcher's three forms: 256 workgroups of 64 x 64 (four channel tiles per wave, the last
        # block partial), one fewer (one tile per wave), and a deep K on that many 64 x 16 tiles
        add(1, (32, 32), 16, 1000, 1, tag="_wide")
        add(1, (30, 32), 16, 1000, 1, tag="_wide")
        add(1, (32, 32), 144, 256, 1, tag="_wide")
        add(1, (1, 1), 1280, 1001, 1, tag="_head")                    # the K split
        add(1, (1, 1), 1280, 1001, 1, bias=False, act="RELU", tag="_head")
        add(3, (2, 2), 1280, 70, 1, tag="_head")                      # M = 12 <= 16, split
        for fill in (127, -127):
            add(2, (1, 1), 1280, 17, 1, w_fill=fill, x_mode="pos", tag="_w%d" % fill)
            add(1, (4, 5), 1280, 17, 1, w_fill=fill, x_mode="neg", tag="_w%d" % fill)
        for act in ACTS:
            add(2, (5, 5), 8, 21, 3, act=act, bias=True)
            add(2, (5, 5), 8, 21, 3, act=act, bias=False)
        # pointers 4 bytes off their buffers: byte / dword fragments, scalar stores
        add(2, (5, 5), 16, 16, 3, in_off=4, q_off=4, out_off=4, tag="_off4")
        add(2, (5, 5), 4, 20, 3, in_off=4, q_off=4, out_off=4, tag="_off4")
        add(1, (1, 1), 1280, 24, 1, in_off=4, q_off=4, out_off=4, tag="_off4")
    return out


def dw_cases():
    out, n = [], 0

    def add(*a, **kw):
        nonlocal n
        n += 1
        kw.setdefault("seed", n)
        kw.setdefault("bias", n % 3 != 0)
        out.append(ConvCase("dw", a[0], a[1], a[2], 0, *a[3:], **kw))
    for c in (1, 3, 4, 5, 16, 130):
        for dm in (1, 2):
            add(1, (5, 6), c, 3, dm=dm)
            add(3, (4, 5), c, 5, stride=2, dm=dm)
    add(2, (9, 8), 8, 3, dilation=2)
    add(2, (9, 8), 6, 3, dilation=2, same=False, dm=2)
    add(3, (7, 7), 12, 3, stride=2, same=False)
    for mode in ("pos", "neg"):
        add(2, (6, 6), 16, 3, x_mode=mode)
        add(2, (6, 6), 5, 3, stride=2, x_mode=mode, dm=2)
    for fill in (127, -127):
        add(2, (6, 6), 8, 5, w_fill=fill, x_mode="pos", tag="_w%d" % fill)
    for act in ACTS:
        add(2, (5, 5), 8, 3, act=act, bias=True)
        add(2, (5, 5), 7, 3, act=act, bias=False)
    add(2, (5, 5), 16, 3, in_off=4, q_off=4, out_off=4, tag="_off4")
    add(2, (5, 5), 6, 3, in_off=4, q_off=4, out_off=4, dm=2, tag="_off4")
    return out


buffer = Y.buffer
_filled = Y._filled


class _Outputs:
    """output buffers filled with a pattern whose surroundings must stay"""

    def __init__(self, device):
        self.device, self.keep = device, []

    def out(self, nbytes, off, word):
        b = buffer(_filled(off + nbytes + SLACK, word), self.device)
        self.keep.append(b)
        return b

    @staticmethod
    def take(buf, nbytes, off, word, dtype, shape):
        got = buf.download(np.uint8, (off + nbytes + SLACK,))
        fill = _filled(off + nbytes + SLACK, word)
        assert (got[:off] == fill[:off]).all(), "bytes in front of the output were written"
        assert (got[off + nbytes:] == fill[off + nbytes:]).all(), "bytes past the output were written"
        return got[off:off + nbytes].copy().view(dtype).reshape(shape)


def _dq_block(o, x, asymmetric, form, in_off, q_off):
    from band_amd import _abi
    B = x.shape[0]
    size = x.size // B
    chunks = (size + CHUNK - 1) // CHUNK
    dx = buffer(np.concatenate([np.zeros(in_off, np.uint8), x.view(np.uint8).reshape(-1)]), o.device)
    dq = o.out(x.size, q_off, 0xa5a5a5a5)
    ds, do = o.out(4 * B, 0, NAN_WORD), o.out(4 * B, 0, 0xa5a5a5a5)
    dp = o.out(8 * B * chunks, 0, NAN_WORD)
    o.keep.append(dx)
    p = _abi.DynQuantItemsParams()
    p.items, p.item_size, p.asymmetric, p.form = B, size, int(asymmetric), form
    p.input, p.q, p.scale, p.offset, p.pairs = dx.value + in_off, dq.value + q_off, ds.value, do.value, dp.value
    return p, dq, ds, do


def _run_dq(p, lib, device, kernel):
    from band_amd import _abi
    assert lib.bh_dynquant_items_kernel(ctypes.byref(p)) == kernel.encode(), lib.bh_last_error()
    if device:
        _abi.check(lib.bh_dynquant_items(ctypes.byref(p), None), "bh_dynquant_items")
    else:
        assert lib.bhx_cpu_dynquant_items(ctypes.byref(p)) == 0, lib.bhx_last_error()


def launch_dq(case, lib, device):
    """the case through bh_dynquant_items (device) or its host twin; returns (q, s, off)"""
    o = _Outputs(device)
    p, dq, ds, do = _dq_block(o, case.x, case.asymmetric, case.form, case.in_off, case.q_off)
    _run_dq(p, lib, device, case.kernel())
    B = case.batch
    return (o.take(dq, case.x.size, case.q_off, 0xa5a5a5a5, np.int8, case.x.shape),
            o.take(ds, 4 * B, 0, NAN_WORD, F, (B,)), o.take(do, 4 * B, 0, 0xa5a5a5a5, np.int32, (B,)))


def pack_filter(case):
    """(the filter as the launcher reads it, k_pad, row sums over all taps int32)"""
    w = case.w
    if case.form == "dw":
        return w.reshape(-1, case.out_c).copy(), 16, w.astype(np.int64).reshape(-1, case.out_c).sum(axis=0).astype(np.int32)
    flat = w.reshape(case.out_c, -1)
    k_pad = (flat.shape[1] + 15) // 16 * 16
    packed = np.zeros((case.out_c, k_pad), np.int8)
    packed[:, :flat.shape[1]] = flat
    return packed, k_pad, flat.astype(np.int64).sum(axis=1).astype(np.int32)


def conv_block(case, ptrs):
    """ConvHybridParams of the case; ptrs: dict of the pointer fields"""
    from band_amd import _abi
    f = _abi.ConvHybridParams()
    g = case.g
    f.batch, (f.in_h, f.in_w), f.in_c = case.batch, case.in_hw, case.in_c
    (f.out_h, f.out_w), f.out_c = g.out_hw, case.out_c
    (f.k_h, f.k_w), (f.stride_h, f.stride_w), (f.dil_h, f.dil_w), (f.pad_h, f.pad_w) = g.k_hw, g.stride, g.dilation, g.pad
    f.depth_multiplier, f.per_channel = case.dm, int(case.form == "pc")
    f.act_min, f.act_max = H.ACT[case.act]
    for k, v in ptrs.items():
        setattr(f, k, v)
    return f


def launch_conv(case, lib, device):
    """The case through bh_dynquant_items + bh_conv2d_hybrid / bh_dwconv2d_hybrid (device) or
    their host twins, the kernel names asserted first.  Returns (q, s, off, y)."""
    from band_amd import _abi
    o = _Outputs(device)
    p, dq, ds, do = _dq_block(o, case.x.reshape(case.batch, -1), case.form != "pt", 0, case.in_off, case.q_off)
    one = case.x.size // case.batch <= ONE_LAUNCH_MAX
    _run_dq(p, lib, device, DQ_ONE if one else DQ_TWO)
    packed, k_pad, sums = pack_filter(case)
    n_out = case.M * case.out_c
    dy = o.out(4 * n_out, case.out_off, NAN_WORD)
    dw, dsum, dws = buffer(packed, device), buffer(sums, device), buffer(case.ws, device)
    db = buffer(case.bias, device) if case.bias is not None else None
    o.keep += [dw, dsum, dws, db]
    f = conv_block(case, dict(q=p.q, in_scale=p.scale, in_offset=p.offset, weights=dw.value, w_row_sum=dsum.value,
                              w_scale=dws.value, bias=db.value if db is not None else None,
                              output=dy.value + case.out_off))
    f.k_pad = k_pad
    dwf = case.form == "dw"
    name = DW_KERNEL if dwf else CONV_KERNEL
    kern = lib.bh_dwconv2d_hybrid_kernel if dwf else lib.bh_conv2d_hybrid_kernel
    assert kern(ctypes.byref(f)) == name.encode(), lib.bh_last_error()
    if device:
        run = lib.bh_dwconv2d_hybrid if dwf else lib.bh_conv2d_hybrid
        _abi.check(run(ctypes.byref(f), None), name)
    else:
        run = lib.bhx_cpu_dwconv_hybrid if dwf else lib.bhx_cpu_conv_hybrid
        assert run(ctypes.byref(f)) == 0, lib.bhx_last_error()
    B = case.batch
    return (o.take(dq, case.x.size, case.q_off, 0xa5a5a5a5, np.int8, case.x.shape),
            o.take(ds, 4 * B, 0, NAN_WORD, F, (B,)), o.take(do, 4 * B, 0, 0xa5a5a5a5, np.int32, (B,)),
            o.take(dy, 4 * n_out, case.out_off, NAN_WORD, F, (B,) + tuple(case.g.out_hw) + (case.out_c,)))


def valid_blocks(ptr):
    """(DynQuantItemsParams, ConvHybridParams for conv, for depthwise) the checks accept, every pointer `ptr`"""
    from band_amd import _abi
    p = _abi.DynQuantItemsParams()
    p.items, p.item_size, p.asymmetric, p.form = 3, 40, 0, 0
    p.input = p.q = p.scale = p.offset = p.pairs = ptr
    case = ConvCase("pc", 2, (5, 5), 4, 8, 3)
    ptrs = {k: ptr for k in ("q", "in_scale", "in_offset", "weights", "w_row_sum", "w_scale", "bias", "output")}
    c = conv_block(case, ptrs)
    c.k_pad = 48
    d = conv_block(ConvCase("dw", 2, (5, 5), 4, 0, 3, dm=2), ptrs)
    d.k_pad = 16
    return p, c, d


DQ_REFUSALS = [("null_input", dict(input=None), "null pointer"), ("null_q", dict(q=None), "null pointer"),
               ("zero_items", dict(items=0), "non-positive extent"), ("negative_size", dict(item_size=-1), "non-positive extent"),
               ("form", dict(form=3), "form must be"),
               ("null_pairs", dict(form=2, pairs=None), "pairs"),
               ("elements", dict(items=1 << 20, item_size=1 << 11), "2^31 or more elements")]
CONV_REFUSALS = [("null_weights", dict(weights=None), "null pointer"), ("null_output", dict(output=None), "null pointer"),
                 ("null_row_sum", dict(w_row_sum=None), "null pointer"), ("null_scale", dict(w_scale=None), "null pointer"),
                 ("zero_out_c", dict(out_c=0), "non-positive extent"), ("zero_batch", dict(batch=0), "non-positive extent"),
                 ("stride", dict(stride_h=0), "non-positive stride or dilation"),
                 ("k", dict(k_h=64, k_w=64, in_c=16, k_pad=65536), "> 65,535"),
                 ("elements", dict(batch=1 << 16, out_h=1 << 8, out_w=1 << 8), "2^31 or more elements"),
                 ("k_pad", dict(k_pad=40), "k_pad")]
DW_REFUSALS = [("null_weights", dict(weights=None), "null pointer"), ("zero_in_h", dict(in_h=0), "non-positive extent"),
               ("multiplier", dict(depth_multiplier=3), "depth_multiplier"),
               ("dilation", dict(dil_w=0), "non-positive stride or dilation"),
               ("elements", dict(batch=1 << 16, out_h=1 << 8, out_w=1 << 8), "2^31 or more elements")]


# ---- models ------------------------------------------------------------------------------
def one_op_model(form, in_shape, out_c=8, k=3, stride=1, act="NONE", padding="SAME", dilation=1, dm=1, bias=True, seed=80):
    """one hybrid CONV_2D ("pt" / "pc") or DEPTHWISE_CONV_2D ("dw") on an input of shape in_shape"""
    g = FGraph(seed=seed, name="hybrid_conv_" + form, hybrid_conv="per_channel")
    x = g.input(list(in_shape))
    if form == "dw":
        y = g.dwconv(x, k=k, stride=stride, act=act, padding=padding, dm=dm, dilation=dilation, hybrid="per_channel")
    else:
        y = g.conv(x, out_c, k=k, stride=stride, act=act, padding=padding, dilation=dilation,
                   hybrid="per_tensor" if form == "pt" else "per_channel")
    if not bias:
        g.mb.ops[-1]["inputs"] = g.mb.ops[-1]["inputs"][:2]
    g.output(y)
    return g.build()


MODELS = {
    "conv_pt_2x7x6x5": lambda: one_op_model("pt", (2, 7, 6, 5), 19, k=3, stride=2, act="RELU6"),
    "conv_pc_2x7x6x5": lambda: one_op_model("pc", (2, 7, 6, 5), 19, k=3, stride=2, act="RELU", bias=False),
    "conv_pc_1x1x1x200_head": lambda: one_op_model("pc", (1, 1, 1, 200), 33, k=1),
    "dw_2x7x6x8": lambda: one_op_model("dw", (2, 7, 6, 8), k=3, stride=1, act="RELU6"),
    "dw_1x6x6x3_dm2": lambda: one_op_model("dw", (1, 6, 6, 3), k=5, stride=2, dm=2, bias=False),
    "mobilenet_v2_32_all": lambda: mobilenet_v2(np.float32, size=32, classes=21, hybrid_conv="per_channel",
                                                hybrid_min_elements=0),
    "mobilenet_v2_32": lambda: mobilenet_v2(np.float32, size=32, classes=21, hybrid_conv="per_channel"),
    "mobilenet_v1_32_all": lambda: mobilenet_v1(np.float32, size=32, classes=21, hybrid_conv="per_channel",
                                                hybrid_min_elements=0),
    "mobilenet_v1_32": lambda: mobilenet_v1(np.float32, size=32, classes=21, hybrid_conv="per_channel"),
    "mobilenet_v1_32_per_tensor": lambda: mobilenet_v1(np.float32, size=32, classes=21, hybrid_conv="per_tensor"),
    "vit_tiny_32": lambda: vit_tiny(np.float32, size=32, dim=48, heads=3, blocks=1, layer_norm=True, mlp=True,
                                    hybrid="symmetric", hybrid_conv="per_channel"),
}
REGISTRATION = lambda: mobilenet_v2(np.float32, size=32, hybrid_conv="per_channel")  # noqa: E731
BATCHED = "mobilenet_v2_32"  # the model of the job-batch and engine tests

model_feed = Y.model_feed


def is_hybrid_conv(om, o):
    return o.builtin in (CONV_2D, DEPTHWISE_CONV_2D) and om.tensors[o.inputs[1]].np_dtype == np.int8


def hybrid_conv_reference(om, o, x):
    """np_conv_hybrid of operator o on input x (the executor's own)"""
    T = om.tensors
    w = T[o.inputs[1]]
    dw = o.builtin == DEPTHWISE_CONV_2D
    out_c = w.shape[3] if dw else w.shape[0]
    assert all(int(z) == 0 for z in w.zero_point) and len(w.scale) in (1, out_c)
    form = "dw" if dw else ("pc" if len(w.scale) > 1 else "pt")
    assert w.quantized_dimension == (3 if dw else 0) or len(w.scale) == 1
    ws = np.full(out_c, w.scale[0], F) if len(w.scale) == 1 else np.asarray(w.scale, F)
    bias = T[o.inputs[2]].data if len(o.inputs) > 2 and o.inputs[2] >= 0 else None
    opt = o.options
    sw, sh = opt.scalar(1, "i", 1), opt.scalar(2, "i", 1)
    dlw, dlh = (opt.scalar(5, "i", 1), opt.scalar(6, "i", 1)) if dw else (opt.scalar(4, "i", 1), opt.scalar(5, "i", 1))
    act = ACTS[opt.scalar(4 if dw else 3, "b", 0)]
    x = np.asarray(x, F).reshape(T[o.inputs[0]].shape)
    g = H.Geom(x.shape[1:3], w.shape[1:3], (sh, sw), (dlh, dlw), opt.scalar(0, "b", 0) == 0)
    return np_conv_hybrid(x, w.data, ws, bias, g, form, act, out_c // x.shape[3] if dw else 1)


# ---- support checks ----------------------------------------------------------------------
def raw_model(depthwise=False, w_dtype=np.int8, w_scale=None, w_zp=None, w_const=True, bias="f32", out_dtype=np.float32,
              in_shape=(1, 4, 4, 8), out_c=8, k=1, filter_in_c=None, stride=1, qdim=None):
    """one CONV_2D / DEPTHWISE_CONV_2D with a float32 input and an 8-bit filter, built field by
    field so that each refusal can be reached; the default is accepted (out_c scales)"""
    from band_amd.tflite_synth import OPT, ModelBuilder, conv_options, dw_options
    mb = ModelBuilder("hybrid_conv_raw")
    x = mb.tensor("x", list(in_shape), np.float32)
    mb.inputs.append(x)
    ins = [x]
    in_c = in_shape[3]
    shape = [1, k, k, out_c] if depthwise else [out_c, k, k, in_c if filter_in_c is None else filter_in_c]
    w_scale = [0.01] * out_c if w_scale is None else list(w_scale)
    w_zp = [0] * len(w_scale) if w_zp is None else list(w_zp)
    wq = dict(scale=w_scale, zero_point=w_zp, qdim=(3 if depthwise else 0) if qdim is None else qdim)
    if w_const:
        ins.append(mb.tensor("w", shape, w_dtype, data=np.ones(shape, w_dtype), **wq))
    else:
        ins.append(mb.tensor("w", shape, w_dtype, **wq))
        mb.inputs.append(ins[-1])
    if bias == "f32":
        ins.append(mb.tensor("b", [out_c], np.float32, data=np.zeros(out_c, np.float32)))
    elif bias == "i32":
        ins.append(mb.tensor("b", [out_c], np.int32, data=np.zeros(out_c, np.int32)))
    elif bias == "input":
        ins.append(mb.tensor("b", [out_c], np.float32))
        mb.inputs.append(ins[-1])
    oq = {} if out_dtype == np.float32 else dict(scale=[0.05], zero_point=[0])
    st = max(stride, 1)
    oh, ow = (in_shape[1] + st - 1) // st, (in_shape[2] + st - 1) // st
    y = mb.tensor("y", [in_shape[0], oh, ow, out_c], out_dtype, **oq)
    if depthwise:
        mb.op("DEPTHWISE_CONV_2D", ins, [y], OPT["DepthwiseConv2DOptions"], dw_options("SAME", stride, "NONE", out_c // in_c))
    else:
        mb.op("CONV_2D", ins, [y], OPT["Conv2DOptions"], conv_options("SAME", stride, "NONE"))
    mb.outputs.append(y)
    return mb.build()


TODAY = "hybrid CONV_2D / DEPTHWISE_CONV_2D (float32 input, int8 filter)"  # the refusal without the flag
HC, HD = "hybrid CONV_2D: ", "hybrid DEPTHWISE_CONV_2D: "
# name -> (builder, the reason with BAND_HIP_HYBRID_CONV=1)
REFUSALS = {}
for _dw, _h in ((False, HC), (True, HD)):
    _n = "dw_" if _dw else "conv_"
    REFUSALS[_n + "uint8_filter"] = (lambda d=_dw: raw_model(d, w_dtype=np.uint8), _h + "uint8 filter")
    REFUSALS[_n + "variable_filter"] = (lambda d=_dw: raw_model(d, w_const=False), _h + "filter must be a constant")
    REFUSALS[_n + "variable_bias"] = (lambda d=_dw: raw_model(d, bias="input"), _h + "bias must be a float32 constant")
    REFUSALS[_n + "int32_bias"] = (lambda d=_dw: raw_model(d, bias="i32"), _h + "bias must be a float32 constant")
    REFUSALS[_n + "int8_output"] = (lambda d=_dw: raw_model(d, out_dtype=np.int8), _h + "float32 output expected")
    REFUSALS[_n + "filter_zero_point"] = (lambda d=_dw: raw_model(d, w_zp=[0, 0, 3, 0, 0, 0, 0, 0]),
                                         _h + "non-zero filter zero point")
    REFUSALS[_n + "scale_count"] = (lambda d=_dw: raw_model(d, w_scale=[0.01] * 3),
                                   _h + "filter scale count is neither 1 nor the output channels")
    REFUSALS[_n + "zero_scale"] = (lambda d=_dw: raw_model(d, w_scale=[0.01] * 7 + [0.0]), _h + "filter scales must be positive")
    REFUSALS[_n + "negative_scale"] = (lambda d=_dw: raw_model(d, w_scale=[-0.01] * 8), _h + "filter scales must be positive")
    REFUSALS[_n + "elements"] = (lambda d=_dw: raw_model(d, in_shape=(1, 1 << 16, 1 << 12, 8)),
                                _h + "a tensor of 2^31 or more elements")
    REFUSALS[_n + "conv_args"] = (lambda d=_dw: raw_model(d, stride=0), "strides must be >= 1")
REFUSALS["conv_grouped"] = (lambda: raw_model(False, filter_in_c=4), HC + "grouped filter")
REFUSALS["conv_k"] = (lambda: raw_model(False, in_shape=(1, 1, 1, 65536), out_c=1), HC + "k_h * k_w * in_c > 65,535")
REFUSALS["dw_one_scale"] = (lambda: raw_model(True, w_scale=[0.01]), HD + "one filter scale")
