"""The fixed-point arithmetic of TFLite's 8-bit kernels, restated once for the
tests: SaturatingRoundingDoublingHighMul, RoundingDivideByPOT,
MultiplyByQuantizedMultiplier, the saturating left shift and TfLiteRound.

Every integer function takes Python ints (arbitrary precision: the table
builders and gemmlowp's inverse square root) or int64 arrays; `mult` / `shift`
/ `e` may then be arrays as well, per channel on the last axis.  The formulas
are written with comparisons as 0 / 1 factors so that one line serves both.

`mutant=` switches one deliberate defect on (tests.directed_harness.MUTANTS);
a name a function does not know leaves it correct, so a caller can hand its
mutant down: "trunc1" belongs to srdhm, "half_up" and "floor2" to rdbypot,
"single" and "no_left" to mbqm, "clamp_first" and "wrap" to the clamp after it
(tests.directed_harness.epilogue_np).

tests/test_fixed_point_cpu.py holds mbqm to the oracle's C code."""
import math
import numbers

import numpy as np

F = np.float32


def _ints(*v):
    """the arguments as Python ints if every one is an integer scalar, else as int64 arrays"""
    if all(isinstance(x, numbers.Integral) for x in v):
        return [int(x) for x in v]
    return [np.asarray(x, np.int64) for x in v]


def srdhm(a, b, mutant=None):
    """SaturatingRoundingDoublingHighMul (never a == b == INT32_MIN here);
    "trunc1": no rounding nudge"""
    a, b = _ints(a, b)
    t = a * b
    if mutant != "trunc1":
        t = t + (1 << 30) - (t < 0) * ((1 << 31) - 1)  # the nudge is 2^30, or 1 - 2^30 below zero
    return (1 - 2 * (t < 0)) * (abs(t) >> 31)  # C++ division truncates toward zero


def rdbypot(x, e, mutant=None):
    """RoundingDivideByPOT: round half away from zero; "half_up": ties go up;
    "floor2": no rounding"""
    x, e = _ints(x, e)
    if mutant == "floor2":
        return x >> e
    if mutant == "half_up":
        return (x + (e > 0) * (1 << (e - (e > 0)))) >> e
    mask = (1 << e) - 1
    return (x >> e) + ((x & mask) > (mask >> 1) + (x < 0))


def mbqm(x, mult, shift, mutant=None):
    """MultiplyByQuantizedMultiplier (shift > 0 is a left shift); "no_left":
    the left shift dropped; "single": one rounding of x M / 2^(31 + e), half
    away from zero"""
    x, mult, shift = _ints(x, mult, shift)
    left, e = shift * (shift > 0), -shift * (shift < 0)
    if mutant == "no_left":
        left = 0 * left
    a = x << left
    if mutant == "single":
        n, t = a * mult, 31 + e
        return (1 - 2 * (n < 0)) * ((abs(n) + (1 << (t - 1))) >> t)
    return rdbypot(srdhm(a, mult, mutant), e, mutant)


def sat_shl(x, e):
    """gemmlowp's SaturatingRoundingMultiplyByPOT for a positive exponent, on a Python int"""
    thr = (1 << (31 - e)) - 1
    return (1 << 31) - 1 if x > thr else (-(1 << 31) if x < -thr else x << e)


def round_half_away(v):
    """TfLiteRound on float32 values, exact"""
    v = np.asarray(v, F)
    t = np.trunc(v)
    return t + np.where(np.abs(v - t) >= F(0.5), np.sign(v), F(0)).astype(F)


def round_half_away64(z):
    """the same rule on one Python float (float64)"""
    return math.copysign(math.floor(abs(z) + 0.5), z)
