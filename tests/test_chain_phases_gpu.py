"""Parity of the raster chain forms (chain_kernel, bh_chain_i8) phase by phase,
on small shapes aimed at the places where each phase's work split can go wrong.
Every case runs in every raster form that bh_chain_lds_bytes admits - px_blocks
4, 2 and 1, with 4, 8 and 16 waves, the deep-issue forms, and the phase-C split
over 2 to 4 workgroups - and is compared bit for bit against the oracle running
the TFLite ops one by one (computed once per case).

Phase A (depthwise): in the 32-pixel form the workgroup deals its channel
groups out wave by wave, every wave covering both pixel blocks; in the other
forms a wave owns one block:
  * ragged tails: a partly filled and an empty block in the last workgroup
    (P = 35 at 5x7; P = 351 at b=3, 9x13);
  * group counts that divide neither the waves nor the groups per round
    (ce 16, 48, 80, 144: 1, 3, 5, 9 groups);
  * out_w < 16 (7, 13): a block spans rows, the column borrow stops at row ends;
  * stride 2 on an odd size (11x10) and dilation 2;
  * batch > 1: a block spans two images.
Phase B / C (the 1x1 GEMMs, whose first load round the 16-pixel forms issue
before the barrier in front of the phase): fewer channel tiles than waves (cout 8 with 16
waves), K of two rounds and a ragged K-step (ce 384, 144), cout not a multiple
of 16 (24, 40), residual together with a stored first output, no second 1x1,
and every split count against 5 channel tiles (ce2 80).
The amortised 64-pixel form (px_blocks 4, second 1x1 K <= 128, >= 8 tiles):
9 and 13 tiles and a partial last tile (ce2 144, 208, 136), first 1x1 K of
96, 144, 192 with cout 24 and 32.
"""
import ctypes

import numpy as np
import pytest

from tests.chain_harness import ChainCase

pytestmark = pytest.mark.gpu

# (px_blocks, waves, deep, c_split)
RASTER_FORMS = ([(px, 4, 0, 0) for px in (4, 2, 1)] + [(1, 8, 0, 0), (1, 16, 0, 0)] +
                [(1, 4, 1, 0), (1, 8, 1, 0), (2, 4, 1, 0)] +
                [(px, w, 0, s) for (px, w) in ((1, 4), (1, 8), (1, 16), (2, 4)) for s in (2, 3, 4)])


def _run_forms(lib, args, must_run=()):
    rng = np.random.default_rng(1 + sum(int(v) for v in args.values()))
    c = ChainCase(rng, **args)
    y_ref, f_ref = c.oracle()
    ran = []
    for px, waves, deep, split in RASTER_FORMS:
        keep = []
        q = c.params(lib, px, keep, waves, 0, 0, deep, split)
        if lib.bh_chain_lds_bytes(ctypes.byref(q)) == 0:
            continue
        y, f = c.gpu(lib, px, waves, 0, 0, deep, split, expect=(y_ref, f_ref))
        tag = "px %d waves %d deep %d split %d" % (px, waves, deep, split)
        if c.store_pw1:
            np.testing.assert_array_equal(y, y_ref, err_msg="first 1x1, " + tag)
        if c.ce2:
            np.testing.assert_array_equal(f, f_ref, err_msg="second 1x1, " + tag)
        ran.append((px, waves, deep, split))
    for form in [(4, 4, 0, 0), (2, 4, 0, 0), (1, 4, 0, 0), (1, 8, 0, 0), (1, 16, 0, 0), (2, 4, 1, 0)] + list(must_run):
        assert form in ran, "form %r not admitted" % (form,)
    return ran


def _case(b, h, w, ce, stride, cout, residual, ce2, **kw):
    return dict(b=b, h=h, w=w, ce=ce, stride=stride, cout=cout, residual=residual, ce2=ce2, **kw)


PHASE_A = [
    _case(1, 5, 7, 16, 1, 8, True, 48),                   # P = 35: blocks of 16, 16, 3, 0; one group
    _case(1, 5, 7, 80, 1, 24, False, 96, fast=False),     # 5 groups over 4 waves, two-step requant
    _case(3, 9, 13, 48, 1, 24, True, 96),                 # P = 351: 16, 15, 0, 0; blocks span images
    _case(3, 9, 13, 144, 1, 24, False, 144),              # 9 groups
    _case(1, 11, 10, 80, 2, 40, False, 128),              # stride 2, odd size: 6 x 5 outputs
    _case(2, 11, 10, 144, 2, 24, True, 144),
    _case(2, 14, 14, 48, 1, 16, True, 96, dil=2),         # dilation 2: the borrow reaches 2 / 4 lanes
    _case(2, 6, 7, 144, 1, 32, False, 64, dil=2),
]

PHASE_BC = [
    _case(2, 7, 7, 64, 1, 8, True, 48),                                   # one tile, up to 16 waves
    _case(1, 7, 7, 384, 1, 64, True, 384, store_pw1=True),                # K = 384: two rounds of K-steps
    _case(1, 7, 7, 144, 1, 24, True, 144, store_pw1=True, fast=False),    # ragged K-step (144 of 192)
    _case(2, 5, 7, 96, 1, 40, False, 80),                                 # cout 40; 5 tiles over 2, 3, 4 slices
    _case(1, 7, 7, 96, 1, 24, True, 80, store_pw1=True),
    _case(1, 7, 7, 96, 1, 24, False, 0),                                  # no second 1x1
    _case(2, 5, 7, 144, 1, 40, True, 0),
]

AMORTISED = [
    _case(2, 9, 9, 96, 1, 24, False, 144),                 # 9 tiles; P = 162: 64, 64, 34
    _case(2, 9, 9, 144, 1, 32, True, 208),                 # 13 tiles; first 1x1 K = 144 (3 K-steps)
    _case(2, 9, 9, 192, 1, 24, True, 136, fast=False),     # partial last tile
    _case(1, 9, 9, 192, 1, 32, False, 144, store_pw1=True),
    _case(1, 9, 9, 96, 1, 32, True, 136),
    _case(1, 9, 9, 144, 1, 24, False, 208),
]


@pytest.mark.parametrize("args", PHASE_A, ids=lambda a: "b%dx%dx%dce%ds%dd%d" % (
    a["b"], a["h"], a["w"], a["ce"], a["stride"], a.get("dil", 1)))
def test_chain_phase_a(gpu_lib, args):
    _run_forms(gpu_lib, args)


@pytest.mark.parametrize("args", PHASE_BC, ids=lambda a: "ce%dco%dce2_%d%s" % (
    a["ce"], a["cout"], a["ce2"], "r" if a["residual"] else ""))
def test_chain_phase_bc(gpu_lib, args):
    ran = _run_forms(gpu_lib, args)
    if args["ce2"] == 80:  # 5 tiles: every split count, none dividing them
        for s in (2, 3, 4):
            assert (1, 4, 0, s) in ran and (1, 8, 0, s) in ran and (2, 4, 0, s) in ran, ran


@pytest.mark.parametrize("args", AMORTISED, ids=lambda a: "ce%dco%dce2_%d" % (a["ce"], a["cout"], a["ce2"]))
def test_chain_amortised(gpu_lib, args):
    _run_forms(gpu_lib, args)
