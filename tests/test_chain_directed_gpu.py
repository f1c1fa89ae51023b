"""Directed parity of the fused kernels: the directed epilogues of
tests/directed_harness.py through ONE stage of a depthwise -> 1x1 [-> ADD] ->
1x1 chain at a time (the other stages random, or pass-through where they feed
the directed one), in every chain form; the fused residual ADD (add_tab) on
every (y, r) pair; bh_irb_i8 under every per-stage requantisation mask.
Bit-exact against the oracle running the ops one by one.

Coverage condition: every kernel name the chain launchers can return -
chain_kernel, chain_persist_kernel, chain_tile_kernel, chain_stage_kernel and
chain_dense_kernel - and, for chain_kernel, each of bh_chain_i8's routes to it
(px_blocks 4 / 2 / 1, 8 and 16 waves, the three deep-issue forms, the phase-C
split) has a form in FORMS.  The chain tests are parametrised over the form; a
case and its oracle are built once per (stage, family, epilogue) and shared by
the forms through a module-scoped cache.
"""
import ctypes

import numpy as np
import pytest

from tests import directed_harness as dh
from tests.chain_harness import ChainCase
from tests.irb_harness import IrbCase
from tests.test_kernels_directed_gpu import RESIDUAL_SETS, passthrough_epi

pytestmark = pytest.mark.gpu

I8 = np.int8
ONE = ((1 << 31) - 1, 0)  # multiplier / shift of a pass-through stage: requant(acc) == acc below 2^30

# (px_blocks, waves, persist, tile, deep, c_split, stage, dense): the selections
# of test_chain_mnv2 (plain, 2 blocks, 8 and 16 waves, the three deep-issue
# forms, the persistent kernel), test_chain_tile_mnv2 (one tile, runs of
# tiles), test_chain_stage_mnv2 (with and without loader waves),
# test_chain_split_phase_c and test_chain_dense
FORMS = {"plain": (4, 4, 0, 0, 0, 0, 0, 0), "plain-8": (1, 8, 0, 0, 0, 0, 0, 0), "deep": (1, 4, 0, 0, 1, 0, 0, 0),
         "tile": (4, 4, 0, 1, 0, 0, 0, 0), "stage": (1, 4, 0, 0, 0, 0, 1, 0), "stage-loaders": (1, 8, 0, 0, 0, 2, 2, 0),
         "split": (1, 4, 0, 0, 0, 2, 0, 0), "dense": (4, 4, 0, 0, 0, 0, 0, 1), "persist": (4, 4, 1, 0, 0, 0, 0, 0),
         "plain-2": (2, 4, 0, 0, 0, 0, 0, 0), "plain-16": (1, 16, 0, 0, 0, 0, 0, 0), "tile-runs": (4, 4, 0, 4, 0, 0, 0, 0),
         "deep-8": (1, 8, 0, 0, 1, 0, 0, 0), "deep-2": (2, 4, 0, 0, 1, 0, 0, 0)}


@pytest.fixture(scope="module")
def cases():
    """directed cases with their oracle outputs, built once and shared by the
    forms: key -> (ChainCase, y_ref, f_ref)"""
    return {}


def directed_chain(stage, epi, residual=False, seed=0):
    """16x16, stride 1: `stage` ("dw" / "pw1" / "pw2") carries the epilogue,
    one triple per channel; the stages before it pass the swept byte through
    unchanged (channel 0; the other channels sit at the zero point), the
    stages after it are random"""
    rng = np.random.default_rng(9500 + seed)
    n = epi.n
    ce, cout, ce2 = {"dw": (n, 16, 32), "pw1": (16, n, 32), "pw2": (16, 16, n)}[stage]
    c = ChainCase(rng, 1, 16, 16, ce, 1, cout, residual, ce2, store_pw1=True)
    sweep = dh._sweep_bytes(I8, 1, ce)[0].reshape(1, 16, 16, ce)
    sigma = dh._sigma(epi, 0)
    bias = dh._bias(epi, sigma).astype(np.int32)
    full = (-128, 127)
    if stage == "dw":
        c.e, c.e_zp, c.d_zp = sweep, epi.in_zp, epi.out_zp
        wd = np.zeros((1, 3, 3, ce), I8)
        wd[0, 1, 1, :] = sigma
        c.wd, c.bd = wd, bias
        c.q["dw"], c.win["dw"] = (epi.mult, epi.shift), (epi.amin, epi.amax)
        return c
    # pass-through depthwise: d = e (e_zp == d_zp, centre tap 1, multiplier one)
    z = epi.in_zp
    e = np.full((1, 16, 16, ce), z, I8)
    e[..., 0] = sweep[..., 0]
    wd = np.zeros((1, 3, 3, ce), I8)
    wd[0, 1, 1, :] = 1
    c.e, c.e_zp, c.d_zp, c.wd, c.bd = e, z, z, wd, np.zeros(ce, np.int32)
    c.q["dw"], c.win["dw"] = (np.full(ce, ONE[0]), np.full(ce, ONE[1])), full
    if stage == "pw1":
        c.wp = c.wp.copy()
        c.wp[:, 0, 0, 0] = sigma
        c.bp, c.p_zp = bias, epi.out_zp
        c.q["pw1"], c.win["pw1"] = (epi.mult, epi.shift), (epi.amin, epi.amax)
        return c
    # pass-through first 1x1: y = d (identity filter, p_zp == d_zp)
    wp = np.zeros((cout, 1, 1, ce), I8)
    wp[np.arange(cout), 0, 0, np.arange(cout)] = 1
    c.wp, c.bp, c.p_zp = wp, np.zeros(cout, np.int32), z
    c.q["pw1"], c.win["pw1"] = (np.full(cout, ONE[0]), np.full(cout, ONE[1])), full
    c.wf = c.wf.copy()
    c.wf[:, 0, 0, 0] = sigma
    c.bf, c.f_zp = bias, epi.out_zp
    c.q["pw2"], c.win["pw2"] = (epi.mult, epi.shift), (epi.amin, epi.amax)
    return c


def run_forms(lib, c, what, want_fast, forms=FORMS, ref=None):
    """every form, by its selection arguments; each must accept the shape.
    want_fast: how many of the three stages must be eligible for the
    single-step requantisation (3: the chain's `fast` is on; 2: off through
    exactly one stage), or None for a chain run both ways.  ref: the case's
    oracle outputs where the caller holds them"""
    from band_amd import _abi
    y_ref, f_ref = c.oracle() if ref is None else ref
    for name, (px, waves, persist, tile, deep, split, stage, dense) in forms.items():
        for fast in ((True, False) if want_fast != 2 else (True,)):
            c.fast = fast
            keep = []
            p = c.params(lib, px, keep, waves, persist, tile, deep, split, stage, (y_ref, f_ref), dense)
            assert lib.bh_chain_lds_bytes(ctypes.byref(p)) > 0, "%s: the %s form refuses the shape" % (what, name)
            if fast and want_fast is not None:
                got = p.dw.requant_fast + p.pw1.requant_fast + p.pw2.requant_fast
                assert got == want_fast, "%s: %d stages eligible" % (what, got)
            _abi.check(lib.bh_chain_i8(ctypes.byref(p), None), "bh_chain_i8")
            y = c._y.download(I8, y_ref.shape)
            f = c._f.download(I8, f_ref.shape)
            del keep
            np.testing.assert_array_equal(y, y_ref, err_msg="%s %s fast %s: first 1x1" % (what, name, fast))
            np.testing.assert_array_equal(f, f_ref, err_msg="%s %s fast %s: second 1x1" % (what, name, fast))


def _stage_case(stage, i, epi):
    c = directed_chain(stage, epi, seed=i)
    y_ref, f_ref = c.oracle()
    if i == 0 and stage != "dw":  # the directed stage's output is the directed epilogue of its accumulators
        got = y_ref if stage == "pw1" else f_ref
        acc = dh.conv_layer(epi, seed=i).acc  # the same sweep order: one image, plane 0
        assert (got.reshape(256, -1) == epi.expect(acc)).all()
    return c, y_ref, f_ref


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("stage", ["dw", "pw1", "pw2"])
@pytest.mark.parametrize("family", ["fast", "two"])
def test_chain_directed_stage(gpu_lib, cases, family, stage, form):
    """the fast triples, then the two-step ones (which switch the chain's
    all-or-nothing `fast` off through this one stage), with the stage's input
    and output zero points at -128, 0 (5) and 127"""
    for i, epi in enumerate(dh.epilogues(family, I8, 9 if stage == "dw" else 16)):
        key = (stage, family, i)
        if key not in cases:
            cases[key] = _stage_case(stage, i, epi)
        c, y_ref, f_ref = cases[key]
        run_forms(gpu_lib, c, "%s %s" % (stage, epi.name), 3 if family == "fast" else 2, {form: FORMS[form]},
                  (y_ref, f_ref))


def _residual_case(i, epi, scales, zps):
    (ys, rs, os_), (r_zp, o_zp) = scales, zps
    c = directed_chain("pw1", epi, residual=True, seed=i)
    c.wp = np.zeros_like(c.wp)
    c.wp[:, 0, 0, 0] = 1
    c.bp = dh._bias(epi, np.ones(epi.n, np.int64)).astype(np.int32)
    c.x = np.ascontiguousarray(np.broadcast_to((np.arange(256) - 128).astype(I8), (1, 16, 16, 256)))
    c.p_s, c.x_s, c.o_s, c.x_zp, c.o_zp = ys, rs, os_, r_zp, o_zp
    c.y_s = os_
    c.residual = False
    y, _ = c.oracle()
    assert all(len(np.unique(y[0, :, :, ch])) == 256 for ch in (0, 255)), "y does not sweep"
    c.residual = True
    return (c,) + c.oracle()


@pytest.mark.parametrize("form", list(FORMS))
def test_chain_residual_every_pair(gpu_lib, cases, form):
    """add_tab on all 65,536 (y, r) pairs: a pass-through first 1x1 of 256
    channels whose output takes every value over the 256 pixels, residual[pixel,
    c] = c - 128, at residual-to-conv scale ratios of 1 / 64, 1 and 64"""
    epi = passthrough_epi()
    for i, ((ys, rs, os_), zps, _) in enumerate(RESIDUAL_SETS):
        key = ("residual", i)
        if key not in cases:
            cases[key] = _residual_case(i, epi, (ys, rs, os_), zps)
        c, y_ref, f_ref = cases[key]
        run_forms(gpu_lib, c, "residual scales %r" % ((ys, rs, os_),), None, {form: FORMS[form]}, (y_ref, f_ref))


@pytest.mark.parametrize("args", [
    dict(b=2, h=9, w=13, cin=24, ce=96, cout=24, stride=1),
    dict(b=1, h=6, w=7, cin=32, ce=32, cout=16, stride=1, has_expand=False),
])
def test_irb_stage_masks(gpu_lib, args):
    """bh_irb_i8's per-stage fast mask (1: expand, 2: depthwise, 4: project):
    all eight values, not only all-on / all-off"""
    rng = np.random.default_rng(len(args) * 7 + args["cin"] + args["cout"])
    c = IrbCase(rng, **args)
    ref = c.oracle()
    keep = []
    c.params(gpu_lib, 1, keep)
    del keep
    assert c.eligible == (7 if c.has_expand else 6), "eligible stages %d" % c.eligible
    for mask in range(8):
        c.fast = mask
        for tile in (1, 2):
            np.testing.assert_array_equal(c.gpu(gpu_lib, tile, expect=ref), ref, err_msg="mask %d tile %d" % (mask, tile))


@pytest.mark.parametrize("family", ["fast", "two"])
def test_irb_directed_depthwise(gpu_lib, family):
    """the directed epilogues through bh_irb_i8's depthwise stage (no expand
    stage: the block input is the swept tensor), a random projection behind it"""
    for i, epi in enumerate(dh.epilogues(family, I8, 9)):
        rng = np.random.default_rng(9700 + i)
        c = IrbCase(rng, 1, 16, 16, epi.n, epi.n, 16, 1, has_expand=False, residual=False)
        sigma = dh._sigma(epi, 0)
        c.x = dh._sweep_bytes(I8, 1, epi.n)[0].reshape(1, 16, 16, epi.n)
        c.x_zp = c.e_zp = epi.in_zp
        wd = np.zeros((1, 3, 3, epi.n), I8)
        wd[0, 1, 1, :] = sigma
        c.wd, c.bd, c.d_zp = wd, dh._bias(epi, sigma).astype(np.int32), epi.out_zp
        c.q["dw"], c.win["dw"] = (epi.mult, epi.shift), (epi.amin, epi.amax)
        ref = c.oracle()
        for fast in (True, False):
            c.fast = fast
            for tile in (1, 2):
                if tile > 1 and not c.supported(gpu_lib, tile):
                    continue
                np.testing.assert_array_equal(c.gpu(gpu_lib, tile, expect=ref), ref, err_msg="%s fast %s tile %d" % (
                    epi.name, fast, tile))
            if fast:
                assert c.eligible & 2 == (2 if family == "fast" else 0), "%s: eligible %d" % (epi.name, c.eligible)
