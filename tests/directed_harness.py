"""Directed int8 / uint8 layers: tensors chosen so that CHOSEN accumulators go
through the real epilogue of every kernel form.

A *triple* is (mult, shift, lo): one output channel requantises the 256
consecutive accumulators lo .. lo + 255 with (mult, shift).  A layer makes
acc[pixel, c] = bias[c] + sigma[c] * (x[pixel] - in_zp): every filter byte
equals the filter zero point except one, which is w_zp + sigma (sigma = +-1),
and the byte under it runs over all 256 values of the type - one 16x16 image
is one sweep.  bias[c] is set so that the sweep is exactly lo .. lo + 255
whatever in_zp and sigma are.  Everything else in the tensors is random: it
must cancel.

Two families, kept apart because bh_conv_requant_fast_ok is per layer:

* fast layers: every channel has 2^30 < mult < 2^31 and a right shift e, and
  (K << 16) + max|bias| + (255 << e) < 2^30 holds.  With e_max the layer's
  largest e the accumulators may use +-budget, budget = 2^30 - (K << 16) -
  (255 << e_max) - 1.  One layer cannot hold every listed e AND tie centres
  near 2^(e + 3): at the largest admissible e (22 for K <= 36) the budget is
  a few million, below 2^23.  So the triples are split over two layers: "low"
  (e in ES, e_max = 20), "top" (e = e_max(K) alone; ties only where one
  fits under the budget) and "small" (e <= 3, so that e = 0 .. 3 meet
  accumulators within 2^20 + 2^12 of 2^30, the 32-bit edge of the identity).
* two-step layers: at least one channel has mult == 2^30, shift == -31 or a
  left shift (int8 only: the legacy uint8 multiplier is below one), so
  fast_ok is 0.  They also carry ordinary right-shift channels with ties, so
  TFLite's two-step form sees the same tie classes.  Their bound is the one
  that keeps the reference defined, |acc| << left < 2^31 - 256 (the output
  zero point is added in int32 as well); for uint8 it is pulled in by 2^24 because the kernels fold the 128-shift of both operands
  into the bias (a term of K * 128 * 255 that TFLite itself never forms).

epilogue_np() restates the epilogue in int64 numpy (tests.fixed_point.mbqm and
the clamp); the CPU test holds it to the oracle on every directed layer, then
uses the same code with a deliberate defect switched on as the mutants.
"""
import functools

import numpy as np

from oracle import runner as orc
from tests.fixed_point import mbqm, srdhm
from tests.kernel_harness import ConvCase

ES = (0, 1, 2, 3, 7, 8, 12, 15, 20)
LEFTS = (1, 2, 7)
# 2^30 + 1, 2^31 - 1, one with its low 20 bits zero, two arbitrary
MULTS = ((1 << 30) + 1, (1 << 31) - 1, 0x5A300000, 1518500250, 1288490189)
MUTANTS = ("half_up", "single", "trunc1", "floor2", "no_left", "clamp_first", "wrap")


def type_range(dtype):
    return (-128, 127) if np.dtype(dtype) == np.int8 else (0, 255)


# --- int64 restatement of the epilogue (and its mutants) --------------------

def epilogue_np(acc, mult, shift, out_zp, amin, amax, dtype, mutant=None):
    """MultiplyByQuantizedMultiplier per channel (last axis), zero point, clamp"""
    v = mbqm(acc, mult, shift, mutant)
    if mutant == "clamp_first":
        out = np.clip(v, amin, amax) + out_zp
    elif mutant == "wrap":
        out = v + out_zp
    else:
        out = np.clip(v + out_zp, amin, amax)
    return out.astype(np.dtype(dtype))  # 8-bit wrap (a no-op for the correct form)


def ties(acc, mult, shift):
    """(positive, negative) step-2 rounding ties: masks over acc"""
    shift = np.asarray(shift, np.int64)
    e = np.maximum(-shift, 0)
    x = srdhm(np.asarray(acc, np.int64) << np.maximum(shift, 0), mult)
    tie = (e > 0) & ((x & ((np.int64(1) << e) - 1)) == (np.int64(1) << np.maximum(e - 1, 0)))
    return tie & (x > 0), tie & (x < 0)


def fast_ok_py(mult, shift, k, max_abs_bias):
    """bh_conv_requant_fast_ok restated (the device test asserts the library agrees)"""
    for m, s in zip(mult, shift):
        if m <= (1 << 30) or s > 0 or s < -30:
            return 0
        if (k << 16) + int(max_abs_bias) + (255 << int(-s)) >= (1 << 30):
            return 0
    return 1


# --- triples ------------------------------------------------------------------

def tie_acc(m, e, sign, scale=3):
    """an accumulator whose step-1 result is a step-2 tie near sign * 2^(e + scale)
    (scale None: the smallest tie, sign * 2^(e - 1)), found with the oracle's own
    tfl_srdhm; None for e == 0 (no ties exist)"""
    if e == 0:
        return None
    x0 = sign * ((1 << (e - 1)) + (0 if scale is None else 1 << (e + scale)))
    guess = (x0 << 31) // m
    tfl_srdhm = orc.lib().tfl_srdhm
    for d in range(-4, 5):
        if -(1 << 31) <= guess + d < (1 << 31) and tfl_srdhm(guess + d, m) == x0:
            return guess + d
    raise AssertionError("no accumulator maps to %d under multiplier %d" % (x0, m))


def e_max(k):
    """largest right shift at which the fast bound leaves room for one sweep"""
    return max(e for e in range(31) if (1 << 30) - (k << 16) - (255 << e) - 1 >= 255)


def fast_budget(k, emax):
    return (1 << 30) - (k << 16) - (255 << emax) - 1


def fast_triples(k, es, n):
    """(mult, shift, lo) arrays of n channels: every multiplier x every e x five
    centres (0, +-budget edge, a positive and a negative tie), padded to n with
    ties further out and sweeps at fractions of the budget"""
    budget = fast_budget(k, max(es))
    out = []

    def put(m, e, lo):
        lo = int(min(max(lo, -budget), budget - 255))
        out.append((m, -e, lo))

    for m in MULTS:
        for e in es:
            put(m, e, -128)
            put(m, e, budget - 255)
            put(m, e, -budget)
            for sign in (1, -1):
                t = tie_acc(m, e, sign)
                # e == 0 has no ties; a tie beyond the budget is replaced by
                # the smallest one (x = +-2^(e - 1)) where that fits
                if t is not None and abs(t) + 128 > budget:
                    t = tie_acc(m, e, sign, scale=None)
                    if abs(t) + 128 > budget:
                        t = None
                put(m, e, (t if t is not None else sign * (8 << e)) - 128)
    assert len(out) <= n, (len(out), n)
    i = 0
    while len(out) < n:
        m, e = MULTS[i % len(MULTS)], es[(i // len(MULTS)) % len(es)]
        sign = 1 if i % 2 == 0 else -1
        t = tie_acc(m, e, sign, scale=5) if e else None
        if t is None or abs(t) + 128 > budget:
            t = sign * (budget // (2 + i))
        put(m, e, t - 128)
        i += 1
    mult, shift, lo = (np.array(v, np.int64) for v in zip(*out))
    return mult, shift, lo


def two_step_triples(dtype, n):
    """mult == 2^30, shift == -31, left shifts (int8), and ordinary right-shift
    channels with ties; sweeps at 0, at both ends of the defined range and at
    ties"""
    signed = np.dtype(dtype) == np.int8
    out = []

    def put(m, s, lo):
        bound = (((1 << 31) - 257) >> max(s, 0)) - (0 if signed else 1 << 24)
        out.append((m, s, int(min(max(lo, -bound), bound - 255))))

    big = 1 << 40
    for e in (0, 1, 5, 12):  # mult == 2^30: every odd accumulator is a step-1 tie
        m = 1 << 30
        for lo in (-128, big, -big, (tie_acc(m, e, 1) or 8) - 128, (tie_acc(m, e, -1) or -8) - 128):
            put(m, -e, lo)
    for m in MULTS + (1 << 30,):  # shift == -31: the result is -1, 0 or 1
        for lo in (-128, big, -big):
            put(m, -31, lo)
        for sign in (1, -1):  # x = +-2^30 is the step-2 tie of e = 31
            put(m, -31, tie_acc(m, 31, sign, scale=None) - 128)
    if signed:
        for left in LEFTS:
            for m in MULTS + (1 << 30,):
                for lo in (-128, big, -big):
                    put(m, left, lo)
    for m in MULTS[:2]:  # ordinary channels: the two-step form on the fast family's ties
        for e in ES + (21, 22, 30):
            put(m, -e, -128)
            put(m, -e, big)
            put(m, -e, -big)
            for sign in (1, -1):
                t = tie_acc(m, e, sign, scale=3 if e <= 22 else None)
                put(m, -e, (t if t is not None else sign * 8) - 128)
    assert len(out) <= n, (len(out), n)
    i = 0
    while len(out) < n:  # more ties, further out
        m, e = MULTS[2 + i % 3], ES[1 + i % (len(ES) - 1)]
        put(m, -e, tie_acc(m, e, 1 if i % 2 else -1, scale=4) - 128)
        i += 1
    mult, shift, lo = (np.array(v, np.int64) for v in zip(*out))
    return mult, shift, lo


class Epi:
    """one directed layer's epilogue: a triple per channel, the output zero
    point and window, and the input zero point the layer is built with"""

    def __init__(self, name, family, dtype, k, mult, shift, lo, out_zp, amin, amax, in_zp):
        self.name, self.family, self.dtype, self.k = name, family, np.dtype(dtype), k
        self.mult, self.shift, self.lo = mult, shift, lo
        self.out_zp, self.amin, self.amax, self.in_zp = out_zp, amin, amax, in_zp
        self.n = len(mult)

    def bound(self):
        """per channel: the largest |acc| the family admits"""
        if self.family == "fast":
            return np.full(self.n, fast_budget(self.k, int(-self.shift.min())), np.int64)
        left = np.maximum(self.shift, 0)
        return (((np.int64(1) << 31) - 257) >> left) - (0 if self.dtype == np.int8 else 1 << 24)

    def take(self, sl):
        e = Epi(self.name, self.family, self.dtype, self.k, self.mult[sl], self.shift[sl], self.lo[sl],
                self.out_zp, self.amin, self.amax, self.in_zp)
        return e

    def expect(self, acc, mutant=None):
        return epilogue_np(acc, self.mult, self.shift, self.out_zp, self.amin, self.amax, self.dtype, mutant)


def windows(dtype):
    """(out_zp, act_min, act_max, in_zp): output zero points at both ends and
    in the middle, the full window and a 41-wide one touching the zero
    point, input zero points at both ends and inside"""
    if np.dtype(dtype) == np.int8:
        return [(-128, -128, 127, -128), (-128, -128, -88, 127), (0, -128, 127, 5), (0, 0, 40, -128),
                (127, -128, 127, 127), (127, 87, 127, -77)]
    # (128 is there so that a quarter of the uint8 outputs stay inside a window:
    # with the zero point at an end, half of every sweep around 0 clamps)
    return [(0, 0, 255, 0), (0, 0, 40, 255), (255, 0, 255, 77), (255, 215, 255, 0), (128, 0, 255, 200)]


@functools.lru_cache(maxsize=None)
def epilogues(family, dtype, k):
    """every directed epilogue of a family at contraction depth k"""
    dtype = np.dtype(dtype)
    out = []
    if family == "fast":
        sets = [("low", fast_triples(k, ES, 256)), ("top", fast_triples(k, (e_max(k),), 32)),
                ("small", fast_triples(k, ES[:4], 128))]
    else:
        sets = [("two", two_step_triples(dtype, 256))]
    for tag, (mult, shift, lo) in sets:
        for zp, amin, amax, in_zp in windows(dtype):
            name = "%s-%s-k%d-%s-zp%d-[%d,%d]" % (family, tag, k, dtype.name, zp, amin, amax)
            out.append(Epi(name, family, dtype, k, mult, shift, lo, zp, amin, amax, in_zp))
    return out


def chunks(epi, n, multiple=1):
    """the epilogue split into layers of at most n channels (a form's channel
    limit), dealt round-robin so that every layer of a two-step epilogue keeps
    channels that make it ineligible; each is padded by repeating its first
    channel up to a multiple of `multiple`"""
    parts = -(-epi.n // n)
    out = []
    for j in range(parts):
        idx = np.arange(j, epi.n, parts)
        pad = -len(idx) % multiple
        idx = np.concatenate([idx, idx[:1].repeat(pad)]) if pad else idx
        part = epi.take(idx)
        if epi.family == "two":
            assert ((part.mult <= 1 << 30) | (part.shift > 0) | (part.shift < -30)).any()
        out.append(part)
    return out


# --- layers ---------------------------------------------------------------------

def _sweep_bytes(dtype, b, planes):
    """(b, 256, planes) bytes: every (image, plane) a different permutation of
    all 256 values of the type"""
    p = np.arange(256)
    img = np.arange(b)[:, None, None]
    pl = np.arange(planes)[None, None, :]
    idx = (p[None, :, None] * (2 * ((img + pl) % 64) + 1) + 7 * pl + 31 * img) % 256
    return (idx + type_range(dtype)[0]).astype(np.dtype(dtype))


def _sigma(epi, w_zp, alternate=True):
    lo, hi = (-127, 127) if epi.dtype == np.int8 else (0, 255)
    s = np.where(np.arange(epi.n) % 2 == 0, 1, -1) if alternate else np.ones(epi.n, np.int64)
    s = np.where(w_zp + s > hi, -1, s)
    return np.where(w_zp + s < lo, 1, s)


def _bias(epi, sigma):
    a = type_range(epi.dtype)[0] - epi.in_zp  # the smallest x - in_zp
    return np.where(sigma > 0, epi.lo - a, epi.lo + 255 + a)


def conv_layer(epi, *, ic=16, k=1, stride=1, dil=1, sweeps=1, w_zp=None, seed=0, **kw):
    """ConvCase whose accumulators are the epilogue's sweeps: the swept byte is
    input channel 0 under the window's centre tap.  .acc holds them, (M, N)."""
    rng = np.random.default_rng(9000 + seed)
    dtype = epi.dtype
    if w_zp is None:
        w_zp = 0
    assert k * k * ic == epi.k, "the fast bound was built for K = %d" % epi.k
    ih = 16 * stride
    c = ConvCase(rng, sweeps, ih, ih, ic, epi.n, k, k, stride=(stride, stride), dil=(dil, dil), dtype=dtype, **kw)
    assert (c.oh, c.ow) == (16, 16)
    sigma = _sigma(epi, w_zp)
    w = np.full((epi.n, k, k, ic), w_zp, np.int64)
    w[:, k // 2, k // 2, 0] += sigma
    sw = _sweep_bytes(dtype, sweeps, 1)[:, :, 0].reshape(sweeps, 16, 16)
    cy = np.arange(16) * stride - c.pad[0] + (k // 2) * dil
    cx = np.arange(16) * stride - c.pad[1] + (k // 2) * dil
    assert cy.min() >= 0 and cy.max() < ih and cx.min() >= 0 and cx.max() < ih
    x = c.x.copy()
    x[:, cy[:, None], cx[None, :], 0] = sw
    bias = _bias(epi, sigma)
    c.x, c.w, c.w_zp, c.bias = x, w.astype(dtype), int(w_zp), bias.astype(np.int32)
    c.in_zp, c.out_zp, c.amin, c.amax = epi.in_zp, epi.out_zp, epi.amin, epi.amax
    c.mult, c.shift = epi.mult.astype(np.int32), epi.shift.astype(np.int32)
    c.epi = epi
    c.acc = bias[None, :] + sigma[None, :] * (sw.reshape(-1, 1).astype(np.int64) - epi.in_zp)
    return c


def dw_layer(epi, *, k=3, dm=1, stride=1, dil=1, w_zp=None, seed=0, **kw):
    """depthwise ConvCase: centre tap w_zp +- 1, the other taps w_zp, every
    input channel swept by its own byte plane"""
    rng = np.random.default_rng(9100 + seed)
    dtype = epi.dtype
    if w_zp is None:
        w_zp = 0
    assert epi.n % dm == 0
    ic = epi.n // dm
    ih = 16 * stride
    c = ConvCase(rng, 1, ih, ih, ic, 0, k, k, stride=(stride, stride), dil=(dil, dil), dtype=dtype,
                 depthwise=True, dm=dm, **kw)
    assert (c.oh, c.ow) == (16, 16)
    sigma = _sigma(epi, w_zp)
    w = np.full((1, k, k, epi.n), w_zp, np.int64)
    w[0, k // 2, k // 2, :] += sigma
    sw = _sweep_bytes(dtype, 1, ic)[0].reshape(16, 16, ic)
    cy = np.arange(16) * stride - c.pad[0] + (k // 2) * dil
    cx = np.arange(16) * stride - c.pad[1] + (k // 2) * dil
    assert cy.min() >= 0 and cy.max() < ih and cx.min() >= 0 and cx.max() < ih
    x = c.x.copy()
    x[0, cy[:, None], cx[None, :], :] = sw
    bias = _bias(epi, sigma)
    c.x, c.w, c.w_zp, c.bias = x, w.astype(dtype), int(w_zp), bias.astype(np.int32)
    c.in_zp, c.out_zp, c.amin, c.amax = epi.in_zp, epi.out_zp, epi.amin, epi.amax
    c.mult, c.shift = epi.mult.astype(np.int32), epi.shift.astype(np.int32)
    c.epi = epi
    per_out = np.repeat(sw.reshape(256, ic).astype(np.int64), dm, axis=1)  # output channel c reads input c // dm
    c.acc = bias[None, :] + sigma[None, :] * (per_out - epi.in_zp)
    return c


def fc_layer(epi, depth, w_zp=0, seed=0):
    """(x, w, bias, acc) of a FULLY_CONNECTED with 256 rows and one unit per
    triple: column 0 of x is swept, column 0 of w is w_zp +- 1"""
    rng = np.random.default_rng(9200 + seed + depth)
    lo, hi = type_range(epi.dtype)
    x = rng.integers(lo, hi + 1, (256, depth)).astype(epi.dtype)
    sw = _sweep_bytes(epi.dtype, 1, 1)[0, :, 0]
    x[:, 0] = sw
    sigma = _sigma(epi, w_zp)
    w = np.full((epi.n, depth), w_zp, np.int64)
    w[:, 0] += sigma
    bias = _bias(epi, sigma)
    acc = bias[None, :] + sigma[None, :] * (sw.astype(np.int64)[:, None] - epi.in_zp)
    return x, w.astype(epi.dtype), bias.astype(np.int32), acc


# --- conditions -------------------------------------------------------------------

def census(cases):
    """what a set of directed layers holds, counted on the oracle's output
    alone: (acc, epi, oracle_out) triples in"""
    r = dict(pos_ties=0, neg_ties=0, at_pos_bound=0, at_neg_bound=0, low=0, high=0, inside=0, total=0,
             es=set(), lefts=set(), accs=0)
    for acc, epi, out in cases:
        out = out.reshape(acc.shape).astype(np.int64)
        tp, tn = ties(acc, epi.mult, epi.shift)
        r["pos_ties"] += int(tp.sum())
        r["neg_ties"] += int(tn.sum())
        b = epi.bound()[None, :]
        r["at_pos_bound"] += int((acc >= b - 255).sum())
        r["at_neg_bound"] += int((acc <= -b + 255).sum())
        r["low"] += int((out == epi.amin).sum())
        r["high"] += int((out == epi.amax).sum())
        r["inside"] += int(((out > epi.amin) & (out < epi.amax)).sum())
        r["total"] += out.size
        r["accs"] += acc.size
        r["es"] |= set(int(-s) for s in epi.shift if s <= 0)
        r["lefts"] |= set(int(s) for s in epi.shift if s > 0)
    return r
