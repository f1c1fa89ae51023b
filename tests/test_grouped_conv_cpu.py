"""Grouped CONV_2D without a GPU: what the workers accept and refuse, CpuConvGrouped
through its C entry point on every case (random, directed, residual ADD, byte
table), one-op models and ShuffleNet-v1 on the kCPU executor, and that dense
models are untouched.  Expected bytes come from the oracle's dense conv per
group (tests/grouped_models.py); every comparison is exact."""
import hashlib

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey, _abi
from band_amd.tflite_reader_py import read
from band_amd.tflite_synth import mobilenet_v2
from tests import grouped_models as G
from tests import reindex_models as R
from tests.graph_reference import run_reference

RANDOM = G.random_cases()
DIRECTED = G.directed_cases()


def _model(buf, mid=0):
    m = HipModel(mid)
    assert m.FromBuffer(buf).ok()
    return m


@pytest.fixture(scope="module")
def refs():
    """random case id -> (case, grouped_ref), the conditions on the reference asserted"""
    out = {}
    for cid, i, dt, act in RANDOM:
        case = G.make_case(i, dt, act)
        ref = G.grouped_ref(case)
        distinct, inside = G.check_reference(case, ref)
        print("%s: %d distinct bytes, %.2f strictly inside the clamp" % (cid, distinct, inside))
        out[cid] = (case, ref)
    return out


# ---- the reference ---------------------------------------------------------------------
def test_reference_is_not_the_dense_conv():
    """grouped_ref differs from a dense conv that sees every input channel (filters
    tiled over the groups) on most bytes: a kernel that ignores groups would show"""
    case = G.make_case(0, np.int8, G.NONE)
    c = case.cc
    ref = G.grouped_ref(case)
    dense = G.orc.conv2d(case.x, np.ascontiguousarray(np.tile(c.w, (1, 1, 1, case.G))), c.bias, in_zp=c.in_zp,
                         w_zp=c.w_zp, out_zp=c.out_zp, mult=c.mult, shift=c.shift, amin=c.amin, amax=c.amax,
                         stride=c.stride, dilation=c.dil, pad=c.pad, out_hw=(c.oh, c.ow))
    assert (dense != ref).mean() > 0.5
    # and from the next group's slice: channel c must read group c // ocg
    rolled = G.GroupedCase(case.shape, np.int8, act=G.NONE, seed=G.seed_of(0, np.int8, G.NONE),
                           x=np.roll(case.x, case.icg, axis=3))
    assert (G.grouped_ref(rolled) != ref).mean() > 0.5


# ---- what the workers accept -------------------------------------------------------------
@pytest.mark.parametrize("dtype", G.DTYPES, ids=["int8", "uint8"])
def test_spec_accepts_grouped_on_both_workers(dtype):
    for i in range(len(G.SHAPES)):
        m = _model(G.one_op_model(G.make_case(i, dtype, G.NONE)))
        spec = HipModelExecutor(0, 0, DeviceFlag.kCPU).InvestigateModelSpec(m)
        assert spec.unsupported_ops[DeviceFlag.kCPU] == set(), i
        assert spec.unsupported_ops[DeviceFlag.kGPU] == set(), i


def _refusals():
    case = G.make_case(0, np.int8, G.NONE)  # ic = 6, G = 2, icg = 3, oc = 10
    return {
        "out_channels": (lambda: G.one_op_model(case, w_shape=(9, 3, 3, 3)),
                         "grouped conv: output channels not a multiple of the group count"),
        "in_channels": (lambda: G.one_op_model(case, w_shape=(10, 3, 3, 4)),
                        "grouped conv: input channels not a multiple of the filter's"),
        "float32": (G.float_grouped_model, "grouped conv: int8 / uint8 only"),
    }


@pytest.mark.parametrize("name", ["out_channels", "in_channels", "float32"])
def test_refusals_say_why(name):
    build, reason = _refusals()[name]
    m = _model(build())
    spec = HipModelExecutor(0, 0, DeviceFlag.kCPU).InvestigateModelSpec(m)
    assert spec.unsupported_ops[DeviceFlag.kCPU] == {0}
    # (the kGPU set is only filled where a GPU is present: tests/test_grouped_conv_gpu.py)
    assert spec.unsupported_ops[DeviceFlag.kGPU] <= {0}
    st = HipModelExecutor(0, 0, DeviceFlag.kCPU).PrepareSubgraph(m)
    assert not st.ok() and reason in st.message(), st.message()


# ---- CpuConvGrouped through the C ABI -----------------------------------------------------
@pytest.mark.parametrize("cid", [c[0] for c in RANDOM])
def test_cpu_launcher_random(refs, cid):
    case, ref = refs[cid]
    np.testing.assert_array_equal(G.launch(case, _abi.load(), False), ref)


@pytest.mark.parametrize("cid,case", DIRECTED, ids=[c[0] for c in DIRECTED])
def test_cpu_launcher_directed(cid, case):
    ref = G.grouped_ref(case)
    G.check_directed(cid, case, ref)
    np.testing.assert_array_equal(G.launch(case, _abi.load(), False), ref)


@pytest.mark.parametrize("cid", [c[0] for c in RANDOM if c[3] == G.NONE])
def test_cpu_launcher_residual_and_table(refs, cid):
    case, ref = refs[cid]
    r, set_add, z, table = G.residual_of(case, ref, 900)
    lib = _abi.load()
    np.testing.assert_array_equal(G.launch(case, lib, False, residual=(r, set_add)), z)
    np.testing.assert_array_equal(G.launch(case, lib, False, table=table).view(np.uint8), table[ref.view(np.uint8)])


def test_cpu_launcher_refuses_bad_groups():
    import ctypes
    lib = _abi.load()
    case = G.make_case(0, np.int8, G.NONE)
    keep = []
    p = G.grouped_params(case, lib, keep, False, groups=4)  # 4 divides neither 6 nor 10
    assert lib.bhx_cpu_conv_grouped(ctypes.byref(p)) != 0
    assert lib.bh_conv2d_grouped_i8_kernel(ctypes.byref(p)) == b""
    p = G.grouped_params(case, lib, keep, False)
    assert lib.bh_conv2d_grouped_i8_kernel(ctypes.byref(p)) == b"conv_grouped_mfma_kernel"


# ---- the kCPU executor ------------------------------------------------------------------------
def non_constant_tensors(buf):
    return [i for i, t in enumerate(read(buf)["tensors"]) if t["data"] is None]


def _run_every_tensor(buf, x, name):
    ref = run_reference(buf, x)
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    assert ex.InvestigateModelSpec(m).unsupported_ops[DeviceFlag.kCPU] == set()
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    key = SubgraphKey(0, 0)
    views = {t: ex.GetTensorView(key, t) for t in non_constant_tensors(buf)}
    ex.GetTensorView(key, ex.GetInputs(key)[0]).GetData()[...] = x
    assert ex.ExecuteSubgraph(key).ok()
    for t, v in views.items():
        np.testing.assert_array_equal(v.GetData().reshape(ref[t].shape), ref[t], err_msg="%s tensor %d" % (name, t))
    return ex, key, ref


@pytest.mark.parametrize("cid", [c[0] for c in RANDOM])
def test_one_op_models_on_cpu_executor(refs, cid):
    """the model carries the case's scales, so the executor derives the case's
    multipliers: run_reference and grouped_ref agree, and the executor with both"""
    case, ref = refs[cid]
    buf = G.one_op_model(case)
    ex, key, vals = _run_every_tensor(buf, case.x, cid)
    np.testing.assert_array_equal(vals[read(buf)["outputs"][0]], ref)
    assert ex.LaunchKernels(key) == ["conv_grouped_host"]


@pytest.mark.parametrize("dtype", G.DTYPES, ids=["int8", "uint8"])
def test_shufflenet_on_cpu_executor_every_tensor(dtype):
    buf = G.shufflenet_small(dtype)
    ops = read(buf)["ops"]
    from oracle.tflite_fb import Model as OModel
    om = OModel(buf)
    assert sum(G.is_grouped(om, o) for o in om.operators) >= 5
    x = R.zoo_input(buf, seed=4)
    ex, key, ref = _run_every_tensor(buf, x, "shufflenet_v1")
    kernels = ex.LaunchKernels(key)
    assert sum(k.startswith("conv_grouped_host") for k in kernels) == sum(G.is_grouped(om, o) for o in om.operators)
    # the activations are alive down to the logits
    assert len(np.unique(ref[om.outputs[0]])) >= 5 and len(ops) > 20


@pytest.mark.parametrize("build", [G.conv_then_add, G.conv_then_relu6], ids=["add", "relu6"])
@pytest.mark.parametrize("dtype", G.DTYPES, ids=["int8", "uint8"])
def test_following_add_and_relu6_on_cpu(build, dtype):
    buf = build(dtype)
    _run_every_tensor(buf, R.zoo_input(buf, seed=6), build.__name__)
    # with only the outputs viewed the ADD / the unary ops fold into the conv
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    assert ex.PrepareSubgraph(m).ok()
    key = SubgraphKey(0, 0)
    x = R.zoo_input(buf, seed=7)
    ref = run_reference(buf, x)
    ex.GetTensorView(key, ex.GetInputs(key)[0]).GetData()[...] = x
    assert ex.ExecuteSubgraph(key).ok()
    t = ex.GetOutputs(key)[0]
    np.testing.assert_array_equal(ex.GetTensorView(key, t).GetData().reshape(ref[t].shape), ref[t])
    kernels = ex.LaunchKernels(key)
    assert len(kernels) == 1 and kernels[0].startswith("conv_grouped_host"), kernels


def test_job_batch_of_3_on_cpu():
    buf = G.conv_then_add(np.int8)
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    assert ex.PrepareSubgraph(m).ok()
    key = SubgraphKey(0, 0)
    st = ex.PrepareJobBatches(m, key, 3)
    assert st.ok(), st.message()
    xs = [R.zoo_input(buf, seed=10 + s) for s in range(3)]
    for s, x in enumerate(xs):
        ex.GetJobSlotView(key, ex.GetInputs(key)[0], 3, s).GetData()[...] = x
    assert ex.ExecuteJobBatch(key, 3).ok()
    for s, x in enumerate(xs):
        ref = run_reference(buf, x)
        for t in ex.GetOutputs(key):
            np.testing.assert_array_equal(ex.GetJobSlotView(key, t, 3, s).GetData().reshape(ref[t].shape), ref[t])


# ---- dense models are untouched -----------------------------------------------------------------
def test_dense_model_has_no_grouped_launch():
    buf = mobilenet_v2(np.int8, size=32, classes=10)
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    assert ex.PrepareSubgraph(m).ok()
    kernels = ex.LaunchKernels(SubgraphKey(0, 0))
    assert kernels and not any("grouped" in k for k in kernels), kernels


def test_synthesiser_default_is_byte_identical():
    """QGraph.conv(groups=1) draws what it drew before groups existed: the hashes
    of mobilenet_v2() computed before the synthesiser learned about groups"""
    assert hashlib.sha256(mobilenet_v2()).hexdigest() == \
        "243142b9c4c948fcdbbb9365fd3eae01bf52013ed7e8fcb40b4bd8a1bc49ce43"
    assert hashlib.sha256(mobilenet_v2(np.uint8)).hexdigest() == \
        "01fa8e1b9e71b4abdd5ac7478ee3a344ea95921fe0901e886352caffa4411153"
