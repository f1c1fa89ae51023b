"""Self-check of tests/float_harness.py: each bound accepts a float32
evaluation of the same op in another summation order (sequential in reverse,
and pairwise) and rejects the mistakes these kernels can make - a tap dropped
at one border pixel, zero padding replaced by edge replication, one channel
of an out_c % 4 tail left at the bias, images of a batch swapped, a pool
divided by f_h f_w instead of the clipped count, a softmax whose maximum is
taken over the first 64 elements only, a NaN clamped to a bound.  The wrong
results are evaluated in float64, so what is rejected is the mistake itself."""
import numpy as np
import pytest

from tests import float_harness as H

f32, f64 = np.float32, np.float64


def data(seed, shape):
    return (np.random.default_rng(seed).uniform(-1, 1, shape) + 0.5).astype(f32)


def normal(seed, shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(f32)


def total(terms, order, dtype):
    """sum over axis 0 in the given order, every partial sum rounded to dtype"""
    terms = [t.astype(dtype) for t in terms]
    if order == "reversed":
        acc = np.zeros_like(terms[0])
        for t in reversed(terms):
            acc = (acc + t).astype(dtype)
        return acc
    while len(terms) > 1:  # pairwise
        nxt = [(terms[i] + terms[i + 1]).astype(dtype) for i in range(0, len(terms) - 1, 2)]
        terms = nxt + ([terms[-1]] if len(terms) % 2 else [])
    return terms[0]


def patches(x, g, mode="constant"):
    """im2col: [n, oh, ow, kh * kw, c], out-of-image taps zero (or edge-replicated)"""
    (kh, kw), (sh, sw), (dh, dw), (ph, pw), (oh, ow) = g.k_hw, g.stride, g.dilation, g.pad, g.out_hw
    hi_h = max(0, (oh - 1) * sh + (kh - 1) * dh + 1 - x.shape[1] - ph)
    hi_w = max(0, (ow - 1) * sw + (kw - 1) * dw + 1 - x.shape[2] - pw)
    xp = np.pad(x, ((0, 0), (ph, hi_h), (pw, hi_w), (0, 0)), mode=mode)
    ys = (np.arange(oh) * sh)[:, None] + (np.arange(kh) * dh)[None, :]
    xs = (np.arange(ow) * sw)[:, None] + (np.arange(kw) * dw)[None, :]
    p = xp[:, ys[:, None, :, None], xs[None, :, None, :], :]
    return p.reshape(x.shape[0], oh, ow, kh * kw, x.shape[3])


def conv_eval(p, w, bias, act, order, dtype, dm=None):
    """p from patches(); w OHWI or [1,kh,kw,c*dm]; sums in the given order and precision"""
    if dm:
        wk = w.reshape(p.shape[3], -1)                                 # [taps][oc]
        terms = [np.repeat(p[:, :, :, t], dm, axis=3).astype(dtype) * wk[t].astype(dtype) for t in range(p.shape[3])]
    else:
        pk = p.reshape(p.shape[:3] + (-1,))                            # [n,oh,ow,K]
        wk = w.reshape(w.shape[0], -1).T                               # [K][oc]
        terms = [pk[..., k, None].astype(dtype) * wk[k].astype(dtype) for k in range(wk.shape[0])]
    y = total(terms, order, dtype)
    if bias is not None:
        y = (y + bias.astype(dtype)).astype(dtype)
    return np.clip(y, *act)


ORDERS = ("reversed", "pairwise")
CONV = dict(x=data(1, (2, 5, 7, 3)), w=normal(2, (5, 3, 3, 3)), bias=normal(3, 5),
            g=H.Geom((5, 7), (3, 3), 2, 1, True))           # K 27, out_c 5: a tail of one channel
DW = dict(x=data(4, (2, 5, 6, 3)), w=normal(5, (1, 3, 3, 6)), bias=normal(6, 6), g=H.Geom((5, 6), (3, 3), 1, 1, True))


@pytest.mark.parametrize("act", ["NONE", "RELU6"])
def test_conv_bound(act):
    x, w, bias, g = CONV["x"], CONV["w"], CONV["bias"], CONV["g"]
    a = H.ACT[act]
    ref, tol = H.conv_ref(x, w, bias, g, a)
    p = patches(x, g)
    np.testing.assert_allclose(conv_eval(p, w, bias, a, "pairwise", f64), ref, rtol=1e-12, atol=1e-12)
    for order in ORDERS:
        assert H.accepts(conv_eval(p, w, bias, a, order, f32), ref, tol), order
    # one tap dropped at one border pixel: with pad 1, pixel (0, 0) sees taps 4, 5, 7, 8 of the 9
    assert g.pad == (1, 1)
    drop = p.copy()
    drop[0, 0, 0, 4, :] = 0
    assert not H.accepts(conv_eval(drop, w, bias, a, "pairwise", f64), ref, tol)
    # zero padding replaced by edge replication
    assert not H.accepts(conv_eval(patches(x, g, "edge"), w, bias, a, "pairwise", f64), ref, tol)
    # the last channel (out_c % 4 == 1) left at the bias
    tail = ref.copy()
    tail[..., -1] = np.clip(bias[-1], *a)
    assert not H.accepts(tail, ref, tol)
    # images of the batch swapped
    assert not H.accepts(ref[::-1], ref, tol)
    if act == "NONE":  # the bound is no looser than a float16 evaluation needs: that must fail
        assert not H.accepts(conv_eval(p, w, bias, a, "pairwise", np.float16), ref, tol)


def test_dwconv_bound():
    x, w, bias, g = DW["x"], DW["w"], DW["bias"], DW["g"]
    a = H.ACT["RELU_N1_TO_1"]
    ref, tol = H.conv_ref(x, w, bias, g, a, depth_multiplier=2)
    p = patches(x, g)
    np.testing.assert_allclose(conv_eval(p, w, bias, a, "pairwise", f64, dm=2), ref, rtol=1e-12, atol=1e-12)
    for order in ORDERS:
        assert H.accepts(conv_eval(p, w, bias, a, order, f32, dm=2), ref, tol), order
    ref, tol = H.conv_ref(x, w, bias, g, H.ACT["NONE"], depth_multiplier=2)
    drop = p.copy()
    drop[1, 4, 5, 0, :] = 0  # the bottom right pixel loses its top left tap
    assert not H.accepts(conv_eval(drop, w, bias, H.ACT["NONE"], "pairwise", f64, dm=2), ref, tol)
    assert not H.accepts(conv_eval(patches(x, g, "edge"), w, bias, H.ACT["NONE"], "pairwise", f64, dm=2), ref, tol)
    wrong_dm = np.repeat(x, 2, axis=3).reshape(x.shape[0], 5, 6, 2, 3).swapaxes(3, 4).reshape(x.shape[0], 5, 6, 6)
    mixed = H.conv_ref(wrong_dm, w, bias, H.Geom((5, 6), (3, 3), 1, 1, True), H.ACT["NONE"], depth_multiplier=1)[0]
    assert not H.accepts(mixed, ref, tol)  # channel c read from input c % in_c instead of c / dm
    assert not H.accepts(ref[::-1], ref, tol)


def test_fc_bound():
    x, w, bias = data(7, (3, 65)), normal(8, (9, 65)), normal(9, 9)
    ref, tol = H.fc_ref(x, w, bias)
    for order in ORDERS:
        terms = [x[:, k, None] * w[None, :, k] for k in range(65)]
        got = (total(terms, order, f32) + bias).astype(f32)
        assert H.accepts(got, ref, tol), order
    short = H.fc_ref(x[:, :64], w[:, :64], bias)[0]   # the 65th element, lane 0's second, dropped
    assert not H.accepts(short, ref, tol)
    tail = ref.copy()
    tail[:, -1] = bias[-1]
    assert not H.accepts(tail, ref, tol)
    assert not H.accepts(ref[::-1], ref, tol)


def test_avg_pool_bound():
    x = data(10, (2, 7, 5, 3))
    g = H.Geom((7, 5), (3, 3), 2, 1, True)
    ref, tol = H.pool_ref(x, "avg", g)
    p = patches(x, g)                                              # zero taps add nothing to the sum
    cnt = patches(np.ones_like(x), g).sum(axis=3)
    assert cnt.min() == 4 and cnt.max() == 9
    for order in ORDERS:
        s = total([p[:, :, :, t] for t in range(9)], order, f32)
        assert H.accepts((s / cnt.astype(f32)).astype(f32), ref, tol), order
    full = total([p[:, :, :, t] for t in range(9)], "pairwise", f64) / 9.0  # divided by f_h f_w
    assert not H.accepts(full, ref, tol)
    assert not H.accepts(ref[::-1], ref, tol)


def test_exact_bounds():
    x = data(11, (2, 7, 5, 3))
    g = H.Geom((7, 5), (3, 3), 2, 1, True)
    ref, tol = H.pool_ref(-x - 1, "max", g)                        # all negative: zero padding would win
    assert tol is None and ref.max() < 0
    assert H.accepts(ref.astype(f32), ref, tol)
    padded = patches(-x - 1, g).max(axis=3)
    assert not H.accepts(padded, ref, tol)
    assert not H.accepts(np.nextafter(ref.astype(f32), f32(0)), ref, tol)
    v = np.array([np.nan, -np.inf, np.inf, -3.0, 0.5, 9.0], f32)
    ref, tol = H.clamp_ref(v, 0.0, 6.0)
    assert np.isnan(ref[0]) and list(ref[1:]) == [0.0, 6.0, 0.0, 0.5, 6.0]
    assert H.accepts(np.clip(v, 0, 6), ref, tol)
    assert not H.accepts(np.fmin(np.fmax(v, f32(0)), f32(6)), ref, tol)   # fminf(fmaxf(NaN, lo), hi) = lo
    ref, tol = H.clamp_ref(v, -np.inf, np.inf)
    assert not H.accepts(np.fmin(np.fmax(v, f32(-np.inf)), f32(np.inf)), ref, tol)  # ... = -inf


def nudge(a, ulps):
    a = np.asarray(a, f32).copy()
    for _ in range(ulps):
        a = np.nextafter(a, f32(np.inf))
    return a


@pytest.mark.parametrize("kind", ["add", "sub", "mul", "sqdiff"])
def test_eltwise_bound(kind):
    a, b = data(12, (2, 5, 7, 6)), normal(13, (1, 1, 1, 6))
    ref, tol = H.eltwise_ref(a, b, kind)
    got = {"add": a + b, "sub": a - b, "mul": a * b, "sqdiff": (a - b) * (a - b)}[kind]
    assert got.dtype == f32 and H.accepts(got, ref, tol)
    assert not H.accepts(nudge(got, 4), ref, tol)
    assert not H.accepts(H.eltwise_ref(a, np.roll(b, 1, axis=3), kind)[0], ref, tol)   # b mis-indexed
    assert not H.accepts(ref[::-1], ref, tol)
    ref6, tol6 = H.eltwise_ref(4 * a, b, kind, H.ACT["RELU6"] if kind != "sub" else H.ACT["RELU_N1_TO_1"])
    assert not H.accepts(H.eltwise_ref(4 * a, b, kind)[0], ref6, tol6)               # the clamp left out


def test_logistic_and_rsqrt_bounds():
    x = np.concatenate([np.linspace(-100, 100, 2001), [0.0, -0.0]]).astype(f32)
    ref, tol = H.logistic_ref(x)
    with np.errstate(over="ignore"):
        got = (f32(1) / (f32(1) + np.exp(-x))).astype(f32)
    assert got.dtype == f32 and H.accepts(got, ref, tol)
    mid = np.abs(x) < 80
    assert not H.accepts(np.where(mid, nudge(got, 6), got), ref, tol)   # gamma(4) |y| is at most 4 ulp
    assert not H.accepts(H.logistic_ref(-x)[0], ref, tol)
    x = np.concatenate([np.logspace(-6, 6, 601), [0.0]]).astype(f32)
    ref, tol = H.rsqrt_ref(x)
    with np.errstate(divide="ignore"):
        got = (f32(1) / np.sqrt(x)).astype(f32)
    assert np.isposinf(ref[-1]) and H.accepts(got, ref, tol)
    assert not H.accepts(nudge(got, 4), ref, tol)                       # gamma(2) |y| is at most 2 ulp
    assert not H.accepts(np.where(np.isinf(got), f32(3.4e38), got), ref, tol)  # +inf must be +inf


@pytest.mark.parametrize("beta", [1.0, 0.8, 3.0])
def test_softmax_bound(beta):
    x = (4 * data(14, (5, 129))).astype(f32)
    x[3] = 1.25
    x[4, 1:] = x[4, 0] - 200.0
    x[1, 100] = x[1, :64].max() + 200.0   # the maximum lies beyond the first 64 elements
    ref, tol = H.softmax_ref(x, f32(beta))
    assert ref[4, 1] < H.FLOOR and ref[4, 1] > 0
    b = f32(beta)

    def soft(mx, order):
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.exp(((x - mx).astype(f32) * b).astype(f32)).astype(f32)
            s = total([e[:, k] for k in range(x.shape[1])], order, f32)[:, None]
            return (e * (f32(1) / s)).astype(f32)
    for order in ORDERS:
        assert H.accepts(soft(x.max(axis=1, keepdims=True), order), ref, tol), order
    first64 = soft(x[:, :64].max(axis=1, keepdims=True), "pairwise")    # expf overflows on row 1
    assert not np.isfinite(first64[1]).all() and not H.accepts(first64, ref, tol)
    assert not H.accepts(ref[::-1], ref, tol)
    skew = H.softmax_ref(x, f32(beta * 1.0001))[0]                       # beta off by 1e-4
    assert not H.accepts(skew, ref, tol)


def test_check_reports_the_ratio(capsys):
    ref = np.array([1.0, 2.0, 4.0])
    assert H.check(np.array([1.0, 2.0 + 1e-7, 4.0]), ref, 4e-7, "probe") == pytest.approx(0.25)
    assert "probe: max |got - ref| / tol = 0.25" in capsys.readouterr().out
    with pytest.raises(AssertionError, match="1 of 3 elements"):
        H.check(np.array([1.0, 2.0, 4.1]), ref, 4e-7, "probe")
    with pytest.raises(AssertionError):
        H.check(np.array([1.0, 2.0]), ref, 1.0, "size")
    assert H.gamma(1) > H.U and H.gamma(45) < 46 * H.U
    assert (H.out_size(True, 8, 3, 2), H.padding(2, 1, 8, 3, 4)) == (4, 0)      # asymmetric: 0 before, 1 after
    assert (H.out_size(False, 9, 3, 1, 2), H.padding(1, 2, 9, 3, 5)) == (5, 0)
    assert (H.out_size(True, 3, 5, 1), H.padding(1, 1, 3, 5, 3)) == (3, 2)
