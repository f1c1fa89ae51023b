"""Hybrid FULLY_CONNECTED (float32 input, int8 weights) without a GPU.

First the numpy restatement of tests/hybrid_models.py alone: against the
float64 product of the dequantised weights at the derived bound, against its
deliberately wrong variants, on the directed tie row and on the directed rows
of the asymmetric form.  Then the host twins (bhx_cpu_dynquant_rows,
bhx_cpu_fc_hybrid) on the launcher cases, bit for bit; the launchers' refusals
(pure host); the models on the kCPU executor with every tensor viewed; job
batches; the support checks' reasons; the synthesiser's old bytes."""
import ctypes
import hashlib

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey, _abi
from band_amd.tflite_synth import OPT, FGraph, ModelBuilder, Table, act_options, attention_block, conv_options, \
    encoder_block, mobilenet_v2
from oracle.tflite_fb import Model as OModel
from tests import float_harness as H
from tests import hybrid_models as Y

F = np.float32
CASES = Y.launcher_cases()
WS = 0.0123


def _model(buf, mid=0):
    m = HipModel(mid)
    assert m.FromBuffer(buf).ok()
    return m


def _random_case(rows, units, depth, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 1, (rows, depth)).astype(F), rng.integers(-127, 128, (units, depth)).astype(np.int8),
            rng.normal(0, 1, units).astype(F))


# ---- the restatement alone -----------------------------------------------------------------
@pytest.mark.parametrize("asym", [False, True], ids=["symmetric", "asymmetric"])
@pytest.mark.parametrize("shape", [(17, 33, 65), (64, 48, 130), (3, 17, 1280), (5, 9, 1)])
def test_reference_within_the_quantisation_bound(shape, asym):
    """|rule - float64 product of the dequantised weights| <= c s ws sum|w| + gamma(3) |y|
    (Y.quantisation_bound); largest error / bound on these cases: 0.26 symmetric, 0.12 asymmetric"""
    x, w, b = _random_case(*shape, seed=5)
    real = Y.real_product(x, w, WS, b)
    got = Y.np_fc_hybrid(x, w, WS, b, "NONE", asym).astype(np.float64)
    tol = Y.quantisation_bound(x, w, WS, asym, real)
    ratio = np.abs(got - real) / tol
    print("hybrid reference %s %s: max error / bound %.3g" % (shape, "asym" if asym else "sym", ratio.max()))
    assert (ratio <= 1.0).all()
    if shape[2] > 1:  # a one-element symmetric row is its own maximum: q = +-127 exactly
        assert ratio.max() > 0.01  # the bound is not vacuous


@pytest.mark.parametrize("shape", [(17, 33, 65), (64, 48, 130)])
@pytest.mark.parametrize("wrong,asym", [("assoc", False), ("assoc", True), ("fma", False), ("fma", True),
                                        ("no_rowsum", True)])
def test_wrong_variants_differ(shape, wrong, asym):
    """each wrong variant changes at least 10 % of the outputs (measured with numpy: (dot s) ws
    0.26 - 0.32, one FMA 0.27 - 0.29, no row-sum term 0.97 - 1.0)"""
    x, w, b = _random_case(*shape, seed=9)
    ref = Y.np_fc_hybrid(x, w, WS, b, "NONE", asym)
    bad = Y.np_fc_hybrid(x, w, WS, b, "NONE", asym, wrong=wrong)
    share = float((ref != bad).mean())
    print("wrong variant %s %s %s: %.3f of the outputs differ" % (wrong, shape, "asym" if asym else "sym", share))
    assert share >= 0.10


def test_half_even_differs_on_exactly_the_ties():
    """[127, k + 0.5 for k in -60 .. 59] has inv == 1; half-to-even moves the 60 ties whose
    half-away value is odd and nothing else"""
    x = Y.TIE_ROW[None, :]
    q, s, off = Y.np_dynquant(x, False)
    qe, _, _ = Y.np_dynquant(x, False, half_even=True)
    assert s[0] == F(1.0) and off[0] == 0 and (F(127.0) / F(127.0)) == F(1.0)
    expect = np.array([127] + [k + 1 if k >= 0 else k for k in range(-60, 60)], np.int8)
    np.testing.assert_array_equal(q[0], expect)
    diff = q[0] != qe[0]
    assert diff.sum() == 60 and not diff[0]
    assert (np.abs(q[0][diff].astype(int)) % 2 == 1).all()


def test_reference_directed_rows():
    """asymmetric: offset -128 on an all-positive row, 127 on an all-negative one, an interior
    value on a mixed one; a zero row gives s = 1 and q = 0; a constant row gives q = 127"""
    rng = np.random.default_rng(3)
    x = rng.normal(0, 1, (5, 40)).astype(F)
    x[0] = np.abs(x[0]) + F(0.25)
    x[1] = -np.abs(x[1]) - F(0.25)
    x[3] = 0
    x[4] = F(0.7)
    q, s, off = Y.np_dynquant(x, True)
    assert off[0] == -128 and off[1] == 127 and -128 < off[2] < 127
    assert s[3] == 1 and off[3] == 0 and (q[3] == 0).all()
    assert (q[4] == 127).all() and off[4] == -128
    assert q[0].min() > -128 and q[0].max() == 127 and q[1].min() == -128
    q, s, off = Y.np_dynquant(x, False)
    assert (off == 0).all() and s[3] == 1 and (q[3] == 0).all() and (q[4] == 127).all()
    assert (np.abs(q.astype(int)).max(axis=1)[[0, 1, 2, 4]] == 127).all() and q.min() >= -127


# ---- the host twins -------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_host_twins(case):
    q, s, off, y = Y.launch(case, _abi.load(), False)
    rq, rs, roff = case.quantised()
    np.testing.assert_array_equal(q, rq, err_msg=case.name + " q")
    np.testing.assert_array_equal(s, rs, err_msg=case.name + " scale")
    np.testing.assert_array_equal(off, roff, err_msg=case.name + " offset")
    np.testing.assert_array_equal(y, case.ref(), err_msg=case.name)


def test_launcher_cases_cover_the_issue():
    assert {c.rows for c in CASES} >= set(Y.ROWS) and {c.units for c in CASES} >= set(Y.UNITS)
    assert {c.depth for c in CASES} >= set(Y.DEPTHS) and {c.act for c in CASES} == set(Y.ACTS)
    pairs = {(c.rows, c.units) for c in CASES}
    assert {(r, u) for r in (15, 16, 17) for u in (15, 16, 17)} <= pairs
    assert {c.asymmetric for c in CASES} == {False, True} and {c.bias is None for c in CASES} == {False, True}
    # the directed asymmetric rows reach both ends and the inside
    offs = np.concatenate([c.quantised()[2] for c in CASES if c.asymmetric])
    assert offs.min() == -128 and offs.max() == 127 and ((offs > -128) & (offs < 127)).any()


def _refusals(lib, who, check, kernel, cpu, blocks, which, cases):
    for name, kw, reason in cases:
        p = blocks()[which]
        assert check(ctypes.byref(p)) == 0, lib.bh_last_error()
        for k, v in kw.items():
            setattr(p, k, v)
        assert check(ctypes.byref(p)) != 0, name
        msg = lib.bh_last_error().decode()
        assert msg.startswith(who + ": ") and reason in msg, msg
        assert kernel(ctypes.byref(p)) == b"", name
        assert cpu(ctypes.byref(p)) != 0, name


def test_launchers_refuse_bad_parameters():
    """bh_dynquant_rows_check / bh_fc_hybrid_check are pure host; the host twins refuse the same"""
    lib = _abi.load()
    keep = Y.AlignedHost(np.zeros(4096, np.uint8))
    blocks = lambda: Y.valid_blocks(keep.value)  # noqa: E731
    _refusals(lib, "bh_dynquant_rows", lib.bh_dynquant_rows_check, lib.bh_dynquant_rows_kernel,
              lib.bhx_cpu_dynquant_rows, blocks, 0, Y.DQ_REFUSALS)
    _refusals(lib, "bh_fc_hybrid", lib.bh_fc_hybrid_check, lib.bh_fc_hybrid_kernel, lib.bhx_cpu_fc_hybrid, blocks, 1,
              Y.FC_REFUSALS)
    assert lib.bh_dynquant_rows_check(None) != 0 and lib.bh_fc_hybrid_check(None) != 0


# ---- models on the kCPU executor ------------------------------------------------------------
def test_hybrid_encoder_block_registers():
    """the hybrid encoder block is in nobody's unsupported_ops and PrepareSubgraph succeeds
    (before hybrid FULLY_CONNECTED: six unsupported ops, 'filter must be a float constant')"""
    m = _model(Y.MODELS[Y.REGISTRATION]())
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    spec = ex.InvestigateModelSpec(m)
    assert spec.unsupported_ops[DeviceFlag.kCPU] == set() and spec.unsupported_ops[DeviceFlag.kGPU] == set()
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()


@pytest.mark.parametrize("name", sorted(Y.MODELS))
def test_models_on_cpu_executor_every_tensor(name):
    buf = Y.MODELS[name]()
    om, runs = H.run_executor(buf, [Y.model_feed(buf, seed=11)], DeviceFlag.kCPU, 0, view_all=True)
    hybrid = sum(Y.is_hybrid_fc(om, o) for o in om.operators)
    assert hybrid >= 1
    assert H.check_graph_ops(om, runs[0], name, gelu_ulps=1)[1]["fc"] == hybrid


def test_launch_kernels_of_a_hybrid_model():
    """two launches per hybrid op on the kCPU executor: the row quantisation, then the product"""
    buf = Y.MODELS["fc_1x130_to_33_symmetric"]()
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    assert ex.PrepareSubgraph(m).ok()
    assert ex.LaunchKernels(SubgraphKey(0, 0)) == ["dynquant_rows_host", "fc_hybrid_host"]


@pytest.mark.parametrize("n", [2, 3])
def test_job_batches_on_cpu(n):
    """each job of a batch equals its own single-job run: every row is quantised alone"""
    buf = Y.MODELS[Y.BATCHED]()
    feeds = [Y.model_feed(buf, seed=20 + s) for s in range(n)]
    om, singles = H.run_executor(buf, feeds, DeviceFlag.kCPU, 0, view_all=False)
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    assert ex.PrepareSubgraph(m).ok()
    key = SubgraphKey(0, 0)
    st = ex.PrepareJobBatches(m, key, 3)
    assert st.ok(), st.message()
    for s in range(n):
        ex.GetJobSlotView(key, ex.GetInputs(key)[0], n, s).GetData()[...] = feeds[s][om.inputs[0]]
    assert ex.ExecuteJobBatch(key, n).ok()
    for s in range(n):
        for t in om.outputs:
            np.testing.assert_array_equal(ex.GetJobSlotView(key, t, n, s).GetData().reshape(singles[s][t].shape),
                                          singles[s][t], err_msg="job %d of %d" % (s, n))


# ---- support checks ---------------------------------------------------------------------------
def _fc(w_dtype=np.int8, w_scale=(0.01,), w_zp=(0,), w_const=True, weights_format=0, bias="f32", out_dtype=np.float32,
        depth=8, units=4):
    mb = ModelBuilder("hybrid_refusal")
    x = mb.tensor("x", [1, depth], np.float32)
    mb.inputs.append(x)
    ins = [x]
    wq = dict(scale=list(w_scale), zero_point=list(w_zp))
    if w_const:
        ins.append(mb.tensor("w", [units, depth], w_dtype, data=np.ones((units, depth), w_dtype), **wq))
    else:
        ins.append(mb.tensor("w", [units, depth], w_dtype, **wq))
        mb.inputs.append(ins[-1])
    if bias == "f32":
        ins.append(mb.tensor("b", [units], np.float32, data=np.zeros(units, np.float32)))
    elif bias == "i32":
        ins.append(mb.tensor("b", [units], np.int32, data=np.zeros(units, np.int32)))
    elif bias == "input":
        ins.append(mb.tensor("b", [units], np.float32))
        mb.inputs.append(ins[-1])
    oq = {} if out_dtype == np.float32 else dict(scale=[0.05], zero_point=[0])
    y = mb.tensor("y", [1, units], out_dtype, **oq)
    opt = act_options("NONE")
    if weights_format:
        opt.set(1, "b", weights_format)
    mb.op("FULLY_CONNECTED", ins, [y], OPT["FullyConnectedOptions"], opt)
    mb.outputs.append(y)
    return mb.build()


def _conv(depthwise):
    mb = ModelBuilder("hybrid_conv")
    x = mb.tensor("x", [1, 4, 4, 8], np.float32)
    mb.inputs.append(x)
    shape = [1, 1, 1, 8] if depthwise else [8, 1, 1, 8]
    w = mb.tensor("w", shape, np.int8, scale=[0.01], zero_point=[0], data=np.ones(shape, np.int8))
    b = mb.tensor("b", [8], np.float32, data=np.zeros(8, np.float32))
    y = mb.tensor("y", [1, 4, 4, 8], np.float32)
    if depthwise:
        from band_amd.tflite_synth import dw_options
        mb.op("DEPTHWISE_CONV_2D", [x, w, b], [y], OPT["DepthwiseConv2DOptions"], dw_options("SAME", 1, "NONE"))
    else:
        mb.op("CONV_2D", [x, w, b], [y], OPT["Conv2DOptions"], conv_options("SAME", 1, "NONE"))
    mb.outputs.append(y)
    return mb.build()


HY = "hybrid FULLY_CONNECTED: "
REFUSALS = {
    "per_channel_scales": (lambda: _fc(w_scale=(0.01,) * 4, w_zp=(0,) * 4), HY + "per-channel filter scales"),
    "filter_zero_point": (lambda: _fc(w_zp=(3,)), HY + "non-zero filter zero point"),
    "uint8_filter": (lambda: _fc(w_dtype=np.uint8, w_zp=(128,)), HY + "uint8 filter"),
    "variable_filter": (lambda: _fc(w_const=False), HY + "filter must be a constant"),
    "weights_format": (lambda: _fc(weights_format=1), HY + "weights_format != 0"),
    "int32_bias": (lambda: _fc(bias="i32"), HY + "bias must be a float constant"),
    "variable_bias": (lambda: _fc(bias="input"), HY + "bias must be a float constant"),
    "int8_output": (lambda: _fc(out_dtype=np.int8), HY + "float32 output expected"),
    "depth": (lambda: _fc(depth=65536, units=1), HY + "depth > 65,535"),
    "conv": (lambda: _conv(False), "hybrid CONV_2D / DEPTHWISE_CONV_2D (float32 input, int8 filter)"),
    "depthwise": (lambda: _conv(True), "hybrid CONV_2D / DEPTHWISE_CONV_2D (float32 input, int8 filter)"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_say_why(name):
    build, reason = REFUSALS[name]
    m = _model(build())
    spec = HipModelExecutor(0, 0, DeviceFlag.kCPU).InvestigateModelSpec(m)
    assert spec.unsupported_ops[DeviceFlag.kCPU] == {0} and spec.unsupported_ops[DeviceFlag.kGPU] == {0}
    st = HipModelExecutor(0, 0, DeviceFlag.kCPU).PrepareSubgraph(m)
    assert not st.ok() and reason in st.message(), st.message()


# ---- the synthesiser ---------------------------------------------------------------------------
def test_float_models_keep_their_bytes():
    """sha256 of three float models built without `hybrid`, recorded on the parent commit"""
    assert hashlib.sha256(encoder_block(np.float32)).hexdigest() == \
        "0dc98cd831d52ff7b7fa340748fc8508d52fde48678d42698b8dd13ed0bf2358"
    assert hashlib.sha256(attention_block(np.float32)).hexdigest() == \
        "853f322b343ab39dc938171c0c115568acc856479bdafd162c55c350ab6839e7"
    assert hashlib.sha256(mobilenet_v2(np.float16, size=32)).hexdigest() == \
        "d8d0fad961785a6bb8f248eac18a77b0ff9a7e44b1f0132e504c8764031caacc"


def test_synthesised_hybrid_op():
    """int8 weights with ws = max|w| / 127 and zero point 0, a plain float32 bias, slot 3 only when asymmetric"""
    for hybrid in ("symmetric", "asymmetric"):
        om = OModel(Y.one_op_model((1, 40), 9, hybrid))
        (o,) = om.operators
        w, b = om.tensors[o.inputs[1]], om.tensors[o.inputs[2]]
        assert w.np_dtype == np.int8 and w.is_const and len(w.scale) == 1 and int(w.zero_point[0]) == 0
        assert np.abs(w.data.astype(int)).max() == 127
        assert b.np_dtype == np.float32 and b.is_const
        assert bool(o.options.scalar(3, "b", 0)) == (hybrid == "asymmetric")
    om = OModel(encoder_block(np.float32, tokens=5, dim=8, heads=2, hidden=16, hybrid="symmetric"))
    assert all(o.name != "DEQUANTIZE" for o in om.operators)
    assert sum(Y.is_hybrid_fc(om, o) for o in om.operators) == 6
    g = FGraph(seed=1)
    with pytest.raises(AssertionError):
        g.fully_connected(g.input([1, 4]), 2, hybrid="per-row")
