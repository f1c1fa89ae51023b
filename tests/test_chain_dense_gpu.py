"""Parity of the dense raster chain form (chain_dense_kernel, bh_chain_params.dense
= 1) on the smallest shapes at which its own splits can go wrong.  Every case
runs in the dense form and in the plain (px_blocks 4, 4 waves) form, and both
are compared bit for bit against the oracle running the TFLite ops one by one
(computed once per case).

The form gives each wave 16 pixels and a slab of LDS of its own for all three
phases, one depthwise channel group and one 1x1 channel tile per load round:
  * ragged and empty blocks: 1x5x7 (P = 35: blocks of 16, 16, 3 and an empty
    one) and 3x9x13 (P = 351, blocks span images);
  * 1, 2, 3 and 9 channel groups (ce 16, 32, 48, 144);
  * stride 2 on 11x10 and dilation 2 on 2x14x14;
  * first 1x1 of one tile (cout 16) and a partial tile (cout 24, 40);
  * K of three steps (ce 144, k_pad 192: a ragged round of two) and of three
    rounds (ce 384);
  * second 1x1 of 6, 9 tiles, a partial last tile (ce2 136) and none (ce2 0);
    its K held in 1, 2 or 5 fragments (cout <= 64, 96, 160);
  * residual together with a stored first output; two-step requantisation.

Interior blocks (INTERIOR): phase A asks, per block of 16 raster-consecutive
pixels, whether every 3x3 tap of every pixel lies inside the image, and then
runs an instantiation of its own that feeds the loaded dwords to the MFMA with
no zero-point select.  Such a block lies within one output row and off both
of its ends, so it needs out_w >= 18: none of the shapes above has one
(dense_blocks() below restates the rule from the case's geometry;
tests/test_chain_dense_blocks_cpu.py pins the counts).  The INTERIOR shapes are
the smallest that have interior blocks beside edge, ragged and - at batch 2 -
image-spanning ones, at stride 1 and 2 and dilation 2, with 1 and 3 channel
groups, a residual together with a stored first output, no second 1x1, both
requantisation forms, and the depthwise input's zero point at -128 and inside.

Narrow 1x1 layers (NARROW): the form admits any out_c % 4 == 0 and every case
above has a multiple of 8.  out_c of 4, 12 and 20 for the first 1x1 and 20
for the second: a single partial channel tile, two tiles with a partial last
one, pixel rows of 1, 3 and 5 four-byte units in the copy-out.
"""
import ctypes

import numpy as np
import pytest

from tests.chain_harness import ChainCase

pytestmark = pytest.mark.gpu


def _case(b, h, w, ce, stride, cout, residual, ce2, **kw):
    return dict(b=b, h=h, w=w, ce=ce, stride=stride, cout=cout, residual=residual, ce2=ce2, **kw)


CASES = [
    _case(1, 5, 7, 16, 1, 16, True, 96),                        # P = 35; one group, one tile, 6 tiles
    _case(3, 9, 13, 48, 1, 24, False, 144),                     # P = 351; 3 groups, partial tile, 9 tiles
    _case(3, 9, 13, 144, 1, 24, True, 144, store_pw1=True),     # 9 groups, K of three steps, residual + stored
    _case(1, 11, 10, 32, 2, 40, False, 136, fast=False),        # stride 2, odd size; partial last tile
    _case(2, 14, 14, 48, 1, 16, True, 96, dil=2),               # dilation 2
    _case(1, 5, 7, 384, 1, 64, True, 96, store_pw1=True),       # K = 384: three rounds of two steps
    _case(1, 5, 7, 32, 1, 64, False, 0),                        # no second 1x1 (a MobileNetV1 pair)
    _case(3, 9, 13, 144, 1, 40, True, 0, fast=False),
    _case(1, 5, 7, 96, 1, 96, False, 48),                       # second 1x1 K = 96: two fragments
    _case(1, 5, 7, 64, 1, 160, True, 32),                       # second 1x1 K = 160: three of five fragments
]


# shapes with interior blocks (b, h, w, stride, dilation: non-empty / interior
# blocks under the harness's SAME padding): 1x3x33 7 / 1, 1x6x35 14 / 4,
# 2x5x21 14 / 2 (one per image), 1x5x67 stride 2 7 / 1, 1x7x37 dilation 2 17 / 3
INTERIOR = [
    _case(1, 3, 33, 16, 1, 16, True, 32, store_pw1=True, e_zp=-128),    # one group; residual + stored
    _case(1, 6, 35, 48, 1, 24, False, 0, fast=False, e_zp=7),           # three groups, no second 1x1, two-step
    _case(2, 5, 21, 48, 1, 8, True, 48, e_zp=-128),                     # blocks span images
    _case(1, 5, 67, 16, 2, 24, False, 40, fast=False, e_zp=-128),       # stride 2: the borrow is off for column 1
    _case(1, 7, 37, 48, 1, 16, True, 32, store_pw1=True, dil=2, e_zp=-19),  # the borrow reaches 2 / 4 lanes
]

NARROW = [
    _case(1, 5, 7, 16, 1, 4, True, 20),                                 # y of 4, f of 20 channels
    _case(1, 5, 7, 32, 1, 12, False, 0),                                # y of 12, no second 1x1
    _case(1, 5, 7, 16, 1, 20, True, 32, store_pw1=True),                # two tiles, the last of 4
    _case(1, 5, 7, 48, 1, 12, False, 20, store_pw1=True, fast=False),
]


def make_case(args):
    """the ChainCase of a CASES / INTERIOR / NARROW entry; e_zp, where given,
    replaces the drawn zero point of the depthwise input"""
    args = dict(args)
    e_zp = args.pop("e_zp", None)
    rng = np.random.default_rng(1 + sum(int(v) for v in args.values()))
    c = ChainCase(rng, **args)
    if e_zp is not None:
        c.e_zp = e_zp
    return c


def dense_blocks(c):
    """The form's interior rule restated from the case's geometry alone: one
    flag per non-empty block of 16 raster-consecutive output pixels, true
    where every pixel exists (m < P) and all nine taps of every pixel - input
    row oy * stride + s * dil - pad_h, column ox * stride + g * dil - pad_w,
    s, g in 0 .. 2 - lie inside the h x w image."""
    P = c.b * c.oh * c.ow
    m = np.arange((P + 15) // 16 * 16)
    valid = m < P
    ox, oy = m % c.ow, m // c.ow % c.oh
    inside = valid.copy()
    for k in range(3):
        y = oy * c.stride + k * c.dil - c.pad[0]
        x = ox * c.stride + k * c.dil - c.pad[1]
        inside &= (y >= 0) & (y < c.h) & (x >= 0) & (x < c.w)
    return inside.reshape(-1, 16).all(axis=1)


def _run(lib, c, dense, expect, eligible=False):
    from band_amd import _abi
    keep = []
    q = c.params(lib, 4, keep, 4, expect=expect, dense=dense)
    assert lib.bh_chain_lds_bytes(ctypes.byref(q)) > 0, "form not admitted (dense %d)" % dense
    if eligible and c.fast:  # the single-step requantisation is what such a case is there for
        assert q.dw.requant_fast and q.pw1.requant_fast and (not c.ce2 or q.pw2.requant_fast), "not eligible"
    _abi.check(lib.bh_chain_i8(ctypes.byref(q), None), "bh_chain_i8")
    y = c._y.download(np.int8, (c.b, c.oh, c.ow, c.cout)) if c._y else None
    f = c._f.download(np.int8, (c.b, c.oh, c.ow, c.ce2)) if c._f else None
    return y, f


def _both_forms(lib, c, eligible=False):
    """dense, then plain, against the oracle (computed once); eligible: a case
    with `fast` on must get the single-step requantisation in every stage"""
    y_ref, f_ref = c.oracle()
    for dense in (1, 0):
        y, f = _run(lib, c, dense, (y_ref, f_ref), eligible)
        tag = "dense form" if dense else "plain form"
        if c.store_pw1:
            np.testing.assert_array_equal(y, y_ref, err_msg="first 1x1, " + tag)
        if c.ce2:
            np.testing.assert_array_equal(f, f_ref, err_msg="second 1x1, " + tag)


def _id(a):
    return "b%dx%dx%dce%ds%dd%dco%dce2_%d%s%s" % (
        a["b"], a["h"], a["w"], a["ce"], a["stride"], a.get("dil", 1), a["cout"], a["ce2"], "r" if a["residual"] else "",
        "" if a.get("fast", True) else "two")


@pytest.mark.parametrize("args", INTERIOR, ids=_id)
def test_chain_dense_interior(gpu_lib, args):
    """cases with blocks on both sides of phase A's interior ballot"""
    c = make_case(args)
    interior = dense_blocks(c)
    assert interior.any(), "no interior block"
    assert not interior.all(), "no edge or ragged block"
    _both_forms(gpu_lib, c, eligible=True)


@pytest.mark.parametrize("args", NARROW, ids=_id)
def test_chain_dense_narrow(gpu_lib, args):
    _both_forms(gpu_lib, make_case(args))


@pytest.mark.parametrize("args", CASES, ids=lambda a: "b%dx%dx%dce%ds%dd%dco%dce2_%d%s" % (
    a["b"], a["h"], a["w"], a["ce"], a["stride"], a.get("dil", 1), a["cout"], a["ce2"], "r" if a["residual"] else ""))
def test_chain_dense(gpu_lib, args):
    _both_forms(gpu_lib, make_case(args))


def test_dense_form_gate(gpu_lib):
    """The form is px_blocks 4 with 4 waves and nothing else beside it."""
    c = ChainCase(np.random.default_rng(3), 1, 5, 7, 32, 1, 16, False, 96)
    for kw, dense, ok in [(dict(), 1, True), (dict(), 2, False), (dict(px_blocks=2), 1, False),
                          (dict(px_blocks=1, waves=8), 1, False), (dict(persist=1), 1, False),
                          (dict(tile=1), 1, False), (dict(deep=1), 1, False), (dict(c_split=2), 1, False),
                          (dict(px_blocks=1, waves=8, stage=1), 1, False)]:
        keep = []
        args = dict(px_blocks=4, waves=4, persist=0, tile=0, deep=0, c_split=0, stage=0)
        args.update(kw)
        q = c.params(gpu_lib, args["px_blocks"], keep, args["waves"], args["persist"], args["tile"], args["deep"],
                     args["c_split"], args["stage"], dense=dense)
        assert (gpu_lib.bh_chain_lds_bytes(ctypes.byref(q)) > 0) == ok, (kw, dense)


@pytest.fixture
def forcedense():
    import os
    old = os.environ.get("BAND_HIP_FUSION")
    os.environ["BAND_HIP_FUSION"] = "forcedense"
    yield
    if old is None:
        del os.environ["BAND_HIP_FUSION"]
    else:
        os.environ["BAND_HIP_FUSION"] = old


@pytest.mark.parametrize("arch", ["mobilenet_v2", "posenet_mobilenet_v1"])
def test_chain_forced_dense_models(gpu_lib, forcedense, arch):
    """Executor level: every feasible chain of a model in the dense form
    (BAND_HIP_FUSION=forcedense) - MobileNetV2's blocks and MobileNetV1's
    depthwise + pointwise pairs - eager, replayed, and job-batched."""
    from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey, tflite_synth as S
    from oracle.runner import OracleInterpreter
    from oracle.tflite_fb import Model as OModel
    assert arch in S.MIX_C3
    buf = getattr(S, arch)(np.int8, size=96)
    om = OModel(buf)
    t = om.tensors[om.inputs[0]]
    rng = np.random.default_rng(5 + len(arch))
    xs = [rng.integers(-128, 128, t.shape).astype(np.int8) for _ in range(3)]
    refs = [OracleInterpreter(om).run({om.inputs[0]: x}) for x in xs]
    m = HipModel(43)
    assert m.FromBuffer(buf).ok()
    ex = HipModelExecutor(43, 1, DeviceFlag.kGPU)
    assert ex.PrepareSubgraph(m).ok()
    key = SubgraphKey(43, 1)
    kernels = [r["kernel"] for r in ex.ProfileSubgraph(key, iters=1)]
    assert "chain_dense_kernel" in kernels, kernels
    for rep in range(2):  # eager, then graph replay
        ex.GetTensorView(key, om.inputs[0]).GetData()[...] = xs[0]
        assert ex.ExecuteSubgraph(key).ok()
        for o in om.outputs:
            got = ex.GetTensorView(key, o).GetData()
            np.testing.assert_array_equal(got, refs[0][o].reshape(got.shape), err_msg="%s run %d" % (arch, rep))
    assert ex.PrepareJobBatches(m, key, 3).ok()
    for s, x in enumerate(xs):
        ex.GetJobSlotView(key, om.inputs[0], 3, s).GetData()[...] = x
    assert ex.ExecuteJobBatch(key, 3).ok()
    for s in range(3):
        for o in om.outputs:
            got = ex.GetJobSlotView(key, o, 3, s).GetData()
            np.testing.assert_array_equal(got, refs[s][o].reshape(got.shape), err_msg="%s slot %d" % (arch, s))
    ex._model_ref = m
