"""Hybrid FULLY_CONNECTED (float32 input, int8 weights) on the MI355X:
dynquant_rows_kernel and fc_hybrid_kernel on the launcher cases of
tests.hybrid_models (kernel names first; the quantised rows, the scales, the
offsets and the outputs bit for bit; the pattern around every output must
stay), the launchers' refusals, and the models through the kGPU executor with
every tensor viewed - an eager pass, then the captured graph twice, each
hybrid op exact against the rule on the executor's own input and every other
op at its float bound - job batches of 2, 3 and 5 against single-job runs, and
a GPU-only engine."""
import ctypes

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey
from tests import float_harness as H
from tests import hybrid_models as Y

pytestmark = pytest.mark.gpu

CASES = Y.launcher_cases()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_launchers(gpu_lib, case):
    q, s, off, y = Y.launch(case, gpu_lib, True)
    rq, rs, roff = case.quantised()
    np.testing.assert_array_equal(q, rq, err_msg=case.name + " q")
    np.testing.assert_array_equal(s, rs, err_msg=case.name + " scale")
    np.testing.assert_array_equal(off, roff, err_msg=case.name + " offset")
    np.testing.assert_array_equal(y, case.ref(), err_msg=case.name)


def _refusals(lib, who, launch, kernel, which, cases, ptr):
    for name, kw, reason in cases:
        p = Y.valid_blocks(ptr)[which]
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
    _refusals(gpu_lib, "bh_dynquant_rows", gpu_lib.bh_dynquant_rows, gpu_lib.bh_dynquant_rows_kernel, 0, Y.DQ_REFUSALS,
              buf.value)
    _refusals(gpu_lib, "bh_fc_hybrid", gpu_lib.bh_fc_hybrid, gpu_lib.bh_fc_hybrid_kernel, 1, Y.FC_REFUSALS, buf.value)


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


def test_hybrid_encoder_block_registers_on_the_gpu_worker(gpu_lib):
    """in nobody's unsupported_ops, PrepareSubgraph succeeds, two launches per hybrid op"""
    buf = Y.MODELS[Y.REGISTRATION]()
    m, ex, key = _exec(buf, 90)
    kernels = ex.LaunchKernels(key)
    assert kernels.count(Y.DQ_KERNEL) == 6 and kernels.count(Y.FC_KERNEL) == 6, kernels
    assert "fc_f32_kernel" not in kernels


@pytest.mark.parametrize("name", sorted(Y.MODELS))
def test_models_gpu_executor_every_tensor(gpu_lib, name):
    """three runs on three inputs: eager, capture, replay"""
    buf = Y.MODELS[name]()
    feeds = [Y.model_feed(buf, seed=30 + i) for i in range(3)]
    om, runs = H.run_executor(buf, feeds, DeviceFlag.kGPU, 1, view_all=True)
    hybrid = sum(Y.is_hybrid_fc(om, o) for o in om.operators)
    assert hybrid >= 1
    for i, vals in enumerate(runs):
        assert H.check_graph_ops(om, vals, "%s run %d" % (name, i), gelu_ulps=16)[1]["fc"] == hybrid


def test_models_job_batches(gpu_lib):
    """jobs of a batch of 2, 3 and 5 equal their own single-job runs: every row is quantised alone"""
    buf = Y.MODELS[Y.BATCHED]()
    feeds = [Y.model_feed(buf, seed=40 + s) for s in range(5)]
    om, singles = H.run_executor(buf, feeds, DeviceFlag.kGPU, 1, view_all=False)
    m, ex, key = _exec(buf, 91)
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


def test_engine_gpu_worker_only_serves_hybrid_encoder_block(gpu_lib, tmp_path):
    """one Band engine whose only worker is a GPU worker registers the hybrid encoder block and answers a
    request with the executor's own result"""
    from band_amd.engine import Engine, JobStatus, Model, SchedulerType, make_config, kBandOk
    buf = Y.MODELS[Y.BATCHED]()
    feed = Y.model_feed(buf, seed=9)
    om, runs = H.run_executor(buf, [feed], DeviceFlag.kGPU, 1, view_all=False)
    e = Engine(make_config([SchedulerType.kRoundRobin], [DeviceFlag.kGPU]))
    path = str(tmp_path / "hybrid_encoder_block.tflite")
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
