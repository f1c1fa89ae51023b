"""The directed layers of tests/directed_harness.py, judged on the CPU by the
oracle alone: what they are guaranteed to contain (ties, accumulators at the
bounds, clamped and unclamped outputs, every shift), and that each of seven
deliberately wrong epilogues differs from the oracle on every layer it can
apply to.  The device tests then only have to be bit-exact on these layers.
"""
import numpy as np
import pytest

from tests import directed_harness as dh
from tests.fixed_point import mbqm

FAMILIES = [(f, d, kind) for f in ("fast", "two") for d in (np.int8, np.uint8) for kind in ("conv", "dw")]


def _layers(family, dtype, kind):
    """[(case, oracle output)] of every directed layer of the family"""
    out = []
    for i, epi in enumerate(dh.epilogues(family, dtype, 16 if kind == "conv" else 9)):
        if kind == "conv":
            c = dh.conv_layer(epi, w_zp=0 if dtype == np.int8 else (0, 255)[i % 2])
        else:
            c = dh.dw_layer(epi, w_zp=0 if dtype == np.int8 else (1, 254)[i % 2])
        out.append((c, c.oracle().reshape(c.acc.shape)))
    return out


_CACHE = {}


def layers(family, dtype, kind):
    key = (family, np.dtype(dtype).name, kind)
    if key not in _CACHE:
        _CACHE[key] = _layers(family, dtype, kind)
    return _CACHE[key]


@pytest.mark.parametrize("family,dtype,kind", FAMILIES)
def test_layers_are_what_they_claim(family, dtype, kind):
    """the sweep of channel c is exactly lo[c] .. lo[c] + 255, the family's
    fast_ok verdict holds, and the int64 restatement equals the oracle"""
    for c, ref in layers(family, dtype, kind):
        e = c.epi
        assert (c.acc.min(0) == e.lo).all() and (c.acc.max(0) == e.lo + 255).all(), e.name
        assert (np.sort(c.acc, axis=0) == e.lo[None, :] + np.arange(256)[:, None]).all(), e.name
        assert (np.abs(c.acc) <= e.bound()[None, :]).all(), e.name
        ok = dh.fast_ok_py(c.mult, c.shift, e.k, int(np.abs(c.bias.astype(np.int64)).max()))
        assert ok == (1 if family == "fast" else 0), e.name
        got = e.expect(c.acc)
        assert (got == ref).all(), "%s: restatement differs from the oracle on %d" % (e.name, (got != ref).sum())


@pytest.mark.parametrize("family,dtype,kind", FAMILIES)
def test_conditions(family, dtype, kind):
    r = dh.census([(c.acc, c.epi, ref) for c, ref in layers(family, dtype, kind)])
    msg = "%s %s %s: %r" % (family, np.dtype(dtype).name, kind, r)
    assert r["pos_ties"] >= 1000 and r["neg_ties"] >= 1000, msg
    assert r["at_pos_bound"] >= 500 and r["at_neg_bound"] >= 500, msg
    assert r["low"] >= 0.05 * r["total"] and r["high"] >= 0.05 * r["total"], msg
    assert r["inside"] >= 0.25 * r["total"], msg
    k = 16 if kind == "conv" else 9
    if family == "fast":
        assert r["es"] == set(dh.ES) | {dh.e_max(k)} and dh.e_max(k) > 20 and not r["lefts"], msg
    else:
        assert r["es"] >= set(dh.ES) | {31} and r["lefts"] == (set(dh.LEFTS) if dtype == np.int8 else set()), msg
        for c, _ in layers(family, dtype, kind):
            assert ((c.mult == 1 << 30) & (c.shift <= 0)).any() and (c.shift == -31).any(), msg
    print(msg)


def _applies(mutant, c, ref):
    """whether a defect can show on a layer at all - decided from the layer's
    parameters and the oracle's output, never from the mutant's"""
    e = c.epi
    if mutant == "half_up":  # differs on negative ties only: negative results must be inside the window
        return e.amin < e.out_zp
    if mutant == "no_left":
        return bool((e.shift > 0).any())
    if mutant == "clamp_first":
        return e.out_zp != 0
    if mutant == "wrap":  # some exact result has to leave the window
        v = mbqm(c.acc, e.mult, e.shift) + e.out_zp
        return bool(((v < e.amin) | (v > e.amax)).any())
    return True  # single, trunc1, floor2: any layer with a right shift


@pytest.mark.parametrize("mutant", dh.MUTANTS)
@pytest.mark.parametrize("family,dtype,kind", FAMILIES)
def test_mutants_differ(family, dtype, kind, mutant):
    applied = 0
    for c, ref in layers(family, dtype, kind):
        if not _applies(mutant, c, ref):
            # only the e_max-only layers with the full window cannot show a
            # wrap (|result| <= 1 there); the other exemptions are by parameter
            assert mutant != "wrap" or "-top-" in c.epi.name, c.epi.name
            continue
        applied += 1
        diff = int((c.epi.expect(c.acc, mutant) != ref).sum())
        assert diff > 0, "%s: mutant %s differs from the oracle on %d of %d outputs" % (
            c.epi.name, mutant, diff, ref.size)
    if mutant == "no_left":
        assert applied == (len(layers(family, dtype, kind)) if (family, dtype) == ("two", np.int8) else 0)
    else:
        assert applied >= 2, "%s applies to %d layers" % (mutant, applied)


def test_half_up_differs_on_negative_ties_only():
    """the round-half-up defect differs from the oracle before the clamp on
    exactly the negative ties (what the directed sets exist to hold)"""
    for c, _ in layers("fast", np.int8, "conv"):
        e = c.epi
        _, neg = dh.ties(c.acc, e.mult, e.shift)
        diff = mbqm(c.acc, e.mult, e.shift) != mbqm(c.acc, e.mult, e.shift, "half_up")
        assert (diff == neg).all(), e.name


def test_fc_layers():
    from oracle import runner as orc
    for dtype, w_zp in ((np.int8, 0), (np.uint8, 1), (np.uint8, 254)):
        for epi in dh.epilogues("two", dtype, 16)[:2]:
            for depth in (16, 37):
                x, w, bias, acc = dh.fc_layer(epi, depth, w_zp)
                ref = orc.fully_connected(x, w, bias, in_zp=epi.in_zp, w_zp=w_zp, out_zp=epi.out_zp,
                                          mult=epi.mult, shift=epi.shift, amin=epi.amin, amax=epi.amax)
                assert (epi.expect(acc) == ref).all(), epi.name


def test_chunks_cover_every_triple():
    for family in ("fast", "two"):
        for epi in dh.epilogues(family, np.uint8, 27):
            parts = dh.chunks(epi, 64, multiple=16)
            assert all(p.n % 16 == 0 and p.n <= 64 for p in parts)
            got = sorted(set(zip(*[np.concatenate([getattr(p, f) for p in parts]) for f in ("mult", "shift", "lo")])))
            assert got == sorted(set(zip(epi.mult, epi.shift, epi.lo)))
            for p in parts:  # a two-step layer stays one after the split
                c = dh.conv_layer(p, ic=3, k=3)
                ok = dh.fast_ok_py(c.mult, c.shift, 27, int(np.abs(c.bias.astype(np.int64)).max()))
                assert ok == (1 if family == "fast" else 0), epi.name
