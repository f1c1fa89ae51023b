"""Hybrid CONV_2D / DEPTHWISE_CONV_2D (float32 input, int8 filter) on the MI355X:
dynquant_item_kernel / dynquant_minmax_kernel + dynquant_items_kernel,
conv_hybrid_kernel and dwconv_hybrid_kernel on the launcher cases of
tests.hybrid_conv_models (kernel names first; the quantised items, the scales,
the offsets and the outputs bit for bit; the pattern around every output must
stay), the launchers' refusals, and the models through kGPU executors built
with BAND_HIP_HYBRID_CONV=1, with outputs only and with every tensor viewed -
an eager pass, then the captured graph twice, each hybrid op exact against the
rule on the executor's own input and every other op at its float bound - job
batches of 2, 3 and 5 against single-job runs, and a GPU-only engine."""
import ctypes

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey
from tests import float_harness as H
from tests import hybrid_conv_models as C

pytestmark = pytest.mark.gpu

DQ_CASES, CONV_CASES, DW_CASES = C.dq_cases(), C.conv_cases(), C.dw_cases()


@pytest.fixture
def hybrid_conv(monkeypatch):
    monkeypatch.setenv("BAND_HIP_HYBRID_CONV", "1")


@pytest.mark.parametrize("case", DQ_CASES, ids=lambda c: c.name)
def test_dynquant_items(gpu_lib, case):
    q, s, off = C.launch_dq(case, gpu_lib, True)
    rq, rs, roff = case.ref()
    np.testing.assert_array_equal(q, rq, err_msg=case.name + " q")
    np.testing.assert_array_equal(s, rs, err_msg=case.name + " scale")
    np.testing.assert_array_equal(off, roff, err_msg=case.name + " offset")


@pytest.mark.parametrize("case", CONV_CASES + DW_CASES, ids=lambda c: c.name)
def test_launchers(gpu_lib, case):
    q, s, off, y = C.launch_conv(case, gpu_lib, True)
    rq, rs, roff = case.quantised()
    np.testing.assert_array_equal(q, rq, err_msg=case.name + " q")
    np.testing.assert_array_equal(s, rs, err_msg=case.name + " scale")
    np.testing.assert_array_equal(off, roff, err_msg=case.name + " offset")
    np.testing.assert_array_equal(y, case.ref(), err_msg=case.name)


def _refusals(lib, who, launch, kernel, which, cases, ptr):
    for name, kw, reason in cases:
        p = C.valid_blocks(ptr)[which]
        assert kernel(ctypes.byref(p)) != b"", lib.bh_last_error()
        for k, v in kw.items():
            setattr(p, k, v)
        assert kernel(ctypes.byref(p)) == b"", name
        assert launch(ctypes.byref(p), None) != 0, name
        msg = lib.bh_last_error().decode()
        assert msg.startswith(who + ": ") and reason in msg, msg
    assert launch(None, None) != 0


def test_launchers_refuse_bad_parameters(gpu_lib):
    from band_amd.device import DeviceBuffer
    buf = DeviceBuffer(4096)
    _refusals(gpu_lib, "bh_dynquant_items", gpu_lib.bh_dynquant_items, gpu_lib.bh_dynquant_items_kernel, 0, C.DQ_REFUSALS,
              buf.value)
    _refusals(gpu_lib, "bh_conv2d_hybrid", gpu_lib.bh_conv2d_hybrid, gpu_lib.bh_conv2d_hybrid_kernel, 1, C.CONV_REFUSALS,
              buf.value)
    _refusals(gpu_lib, "bh_dwconv2d_hybrid", gpu_lib.bh_dwconv2d_hybrid, gpu_lib.bh_dwconv2d_hybrid_kernel, 2,
              C.DW_REFUSALS, buf.value)


# ---- models ------------------------------------------------------------------------------
def _exec(buf, mid):
    m = HipModel(mid)
    assert m.FromBuffer(buf).ok()
    ex = HipModelExecutor(mid, 1, DeviceFlag.kGPU)
    spec = ex.InvestigateModelSpec(m)
    assert spec.unsupported_ops[DeviceFlag.kGPU] == set(), spec.unsupported_ops
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    ex._model_ref = m
    return m, ex, SubgraphKey(mid, 1)


def test_dynamic_range_mobilenet_registers_on_the_gpu_worker(gpu_lib, hybrid_conv):
    """in nobody's unsupported_ops, PrepareSubgraph succeeds, a quantisation launch and a product launch
    per hybrid op (filters under 1024 elements - the first conv, the narrow depthwise ones - stay float32)"""
    from oracle.tflite_fb import Model as OModel
    buf = C.REGISTRATION()
    om = OModel(buf)
    convs = sum(C.is_hybrid_conv(om, o) and o.builtin == C.CONV_2D for o in om.operators)
    dws = sum(C.is_hybrid_conv(om, o) and o.builtin == C.DEPTHWISE_CONV_2D for o in om.operators)
    m, ex, key = _exec(buf, 92)
    kernels = ex.LaunchKernels(key)
    assert kernels.count(C.CONV_KERNEL) == convs >= 30 and kernels.count(C.DW_KERNEL) == dws >= 1, kernels
    assert kernels.count(C.DQ_ONE) == convs + dws, kernels


def test_flag_unset_refuses_on_the_gpu_worker(gpu_lib, monkeypatch):
    monkeypatch.delenv("BAND_HIP_HYBRID_CONV", raising=False)
    m = HipModel(93)
    assert m.FromBuffer(C.MODELS["conv_pc_2x7x6x5"]()).ok()
    ex = HipModelExecutor(93, 1, DeviceFlag.kGPU)
    assert ex.InvestigateModelSpec(m).unsupported_ops[DeviceFlag.kGPU] == {0}
    st = ex.PrepareSubgraph(m)
    assert not st.ok() and st.message().endswith(": " + C.TODAY), st.message()


@pytest.mark.parametrize("view_all", [True, False], ids=["every_tensor", "outputs"])
@pytest.mark.parametrize("name", sorted(C.MODELS))
def test_models_gpu_executor(gpu_lib, hybrid_conv, name, view_all):
    """three runs on three inputs: eager, capture, replay.  With outputs only, the outputs equal
    those of the every-tensor run's rule-checked graph: compared with a second executor's"""
    buf = C.MODELS[name]()
    feeds = [{t: v * np.float32(1 + i) for t, v in C.model_feed(buf, seed=30 + i).items()} for i in range(3)]
    om, runs = H.run_executor(buf, feeds, DeviceFlag.kGPU, 1, view_all=view_all)
    hybrid = sum(C.is_hybrid_conv(om, o) for o in om.operators)
    assert hybrid >= 1
    if view_all:
        for i, vals in enumerate(runs):
            assert H.check_graph_ops(om, vals, "%s run %d" % (name, i), gelu_ulps=16)[1]["conv"] == hybrid
        return
    _, full = H.run_executor(buf, feeds, DeviceFlag.kGPU, 1, view_all=True)
    for i, vals in enumerate(runs):
        for t in om.outputs:
            assert np.isfinite(vals[t]).all()
            np.testing.assert_array_equal(vals[t], full[i][t], err_msg="%s run %d" % (name, i))


def test_models_job_batches(gpu_lib, hybrid_conv):
    """jobs of a batch of 2, 3 and 5 equal their own single-job runs: every item is quantised alone"""
    buf = C.MODELS[C.BATCHED]()
    feeds = [{t: v * np.float32(1 + 2 * s) for t, v in C.model_feed(buf, seed=40 + s).items()} for s in range(5)]
    om, singles = H.run_executor(buf, feeds, DeviceFlag.kGPU, 1, view_all=False)
    m, ex, key = _exec(buf, 94)
    st = ex.PrepareJobBatches(m, key, 5)
    assert st.ok(), st.message()
    assert ex.MaxJobBatch(key) == 5
    t_in = ex.GetInputs(key)[0]
    for n in (2, 3, 5):
        order = [(s + n) % 5 for s in range(n)]
        for s, i in enumerate(order):
            ex.GetJobSlotView(key, t_in, n, s).GetData()[...] = feeds[i][om.inputs[0]]
        for _ in range(2):
            assert ex.ExecuteJobBatch(key, n).ok()
            for s, i in enumerate(order):
                for t in om.outputs:
                    got = ex.GetJobSlotView(key, t, n, s).GetData()
                    np.testing.assert_array_equal(got.reshape(singles[i][t].shape), singles[i][t],
                                                  err_msg="n=%d slot %d" % (n, s))


def test_engine_gpu_worker_only_serves_dynamic_range_mobilenet(gpu_lib, hybrid_conv, tmp_path):
    """one Band engine whose only worker is a GPU worker registers the dynamic-range MobileNetV2 and
    answers a request with the executor's own result"""
    from band_amd.engine import Engine, JobStatus, Model, SchedulerType, make_config, kBandOk
    buf = C.MODELS[C.BATCHED]()
    feed = C.model_feed(buf, seed=9)
    om, runs = H.run_executor(buf, [feed], DeviceFlag.kGPU, 1, view_all=False)
    e = Engine(make_config([SchedulerType.kRoundRobin], [DeviceFlag.kGPU]))
    path = str(tmp_path / "dynamic_range_mobilenet_v2.tflite")
    with open(path, "wb") as f:
        f.write(buf)
    m = Model()
    assert m.FromPath(path)
    assert e.RegisterModel(m)
    t = e.CreateInputTensor(m, 0)
    t.data()[...] = feed[om.inputs[0]]
    outs = [e.CreateOutputTensor(m, 0)]
    h = e.RequestAsync(m, [t])
    assert h >= 0 and e.Wait(h, outs) == kBandOk
    assert e.GetJobRecord(h).status == JobStatus.kSuccess
    ref = runs[0][om.outputs[0]]
    assert np.isfinite(ref).all()
    np.testing.assert_array_equal(outs[0].data().reshape(ref.shape), ref)
