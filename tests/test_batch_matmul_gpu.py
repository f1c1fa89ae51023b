"""BATCH_MATMUL on the MI355X: bh_batch_matmul_i8 on every case of
tests.bmm_models.launcher_cases in both requantisation forms (each asserts the
kernel name first; the 0xff bytes past the output must stay), the refused
parameter sets, bh_batch_matmul_f32, and attention_block / vit_tiny through
the kGPU executor (eager and replayed, outputs only and every tensor viewed,
job batches 2, 3, 5) and the engine.

Reference: tests.bmm_models.bmm_ref (the oracle's FULLY_CONNECTED per batch
slice; float64 with the bound gamma(K + 2) sum|a||b| + 2^-126 for floats) and
run_reference for models.  int8 tensors are compared with assert_array_equal,
float model tensors at the tolerance of tests/test_float_cpu.py."""
import ctypes

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey
from oracle.tflite_fb import Model as OModel
from tests import bmm_models as B
from tests import float_harness as H
from tests import reindex_models as R
from tests.graph_reference import run_reference
from tests.test_float_cpu import assert_float_close

pytestmark = pytest.mark.gpu

CASES = B.launcher_cases()
FLOAT_CASES = B.float_cases()


@pytest.fixture(scope="module")
def refs():
    return {c.name: B.bmm_ref(c) for c in CASES + FLOAT_CASES}


@pytest.mark.parametrize("fast", [0, 1], ids=["two_step", "single_step"])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_batch_matmul_launcher(gpu_lib, refs, case, fast):
    """fast = 1 asks for the single-step form; the launcher takes it where
    bh_conv_requant_fast_ok holds and the two-step form otherwise"""
    probe = B.bmm_params(case, 256, 256, 256, fast)
    assert gpu_lib.bh_batch_matmul_i8_kernel(ctypes.byref(probe)) == B.KERNEL.encode()
    got = B.launch(case, gpu_lib, device=True, requant_fast=fast)
    np.testing.assert_array_equal(got, refs[case.name], err_msg="%s fast_ok=%d" % (case.name, B.fast_ok(case, gpu_lib)))


def test_launcher_decides_the_form_itself(gpu_lib, refs):
    """requant_fast = -1 on a case of each form"""
    for name in ("clamps", "left_shift", "ties_k33"):
        case = next(c for c in CASES if c.name == name)
        np.testing.assert_array_equal(B.launch(case, gpu_lib, device=True, requant_fast=-1), refs[name], err_msg=name)


@pytest.mark.parametrize("name,change,reason", B.refused_params(), ids=[r[0] for r in B.refused_params()])
def test_batch_matmul_refuses_bad_parameters(gpu_lib, name, change, reason):
    from band_amd.device import DeviceBuffer
    bufs = [DeviceBuffer(256) for _ in range(3)]
    p = B.valid_params(*(b.value for b in bufs))
    assert gpu_lib.bh_batch_matmul_i8_kernel(ctypes.byref(p)) == B.KERNEL.encode()
    change(p)
    assert gpu_lib.bh_batch_matmul_i8_kernel(ctypes.byref(p)) == b""
    assert gpu_lib.bh_batch_matmul_i8(ctypes.byref(p), None) != 0
    msg = gpu_lib.bh_last_error().decode()
    assert msg.startswith("bh_batch_matmul_i8: ") and reason in msg, msg
    if name != "k_limit":
        assert gpu_lib.bh_batch_matmul_f32(ctypes.byref(p), None) != 0
        assert gpu_lib.bh_last_error().decode().startswith("bh_batch_matmul_f32: ")
    assert gpu_lib.bh_batch_matmul_i8(None, None) != 0


@pytest.mark.parametrize("case", FLOAT_CASES, ids=[c.name for c in FLOAT_CASES])
def test_batch_matmul_f32_launcher(gpu_lib, refs, case):
    ref, tol = refs[case.name]
    H.check(B.launch(case, gpu_lib, device=True), ref, tol, case.name)


# ---- models --------------------------------------------------------------------------
def _exec(buf, mid):
    m = HipModel(mid)
    assert m.FromBuffer(buf).ok()
    ex = HipModelExecutor(mid, 1, DeviceFlag.kGPU)
    assert ex.InvestigateModelSpec(m).unsupported_ops[DeviceFlag.kGPU] == set()  # registers whole on the GPU
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    ex._model_ref = m
    return m, ex, SubgraphKey(mid, 1)


def _compare(name, t, got, ref):
    assert got.dtype == ref.dtype, (name, t)
    if ref.dtype == np.float32:
        assert_float_close(got, ref, "%s tensor %d" % (name, t))
    else:
        np.testing.assert_array_equal(got.reshape(ref.shape), ref, err_msg="%s tensor %d" % (name, t))


@pytest.fixture(scope="module")
def model_refs():
    """per model: its bytes, 5 inputs and run_reference of each"""
    out = {}
    for name, build in B.MODELS.items():
        buf = build()
        xs = [R.zoo_input(buf, seed=40 + i) for i in range(5)]
        out[name] = (buf, xs, [run_reference(buf, x) for x in xs])
    return out


@pytest.mark.parametrize("all_tensors", [False, True], ids=["outputs", "every_tensor"])
@pytest.mark.parametrize("name", sorted(B.MODELS))
def test_models_gpu_executor(gpu_lib, monkeypatch, model_refs, name, all_tensors):
    """an eager pass, then the captured graph twice; with only the outputs
    viewed and with every non-constant tensor viewed (the scores included)"""
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf, xs, refs_ = model_refs[name]
    m, ex, key = _exec(buf, 71)
    om = OModel(buf)
    kernels = [r["kernel"] for r in ex.ProfileSubgraph(key, iters=1)]
    want = "bmm_f32_kernel" if name == "attention_f32" else B.KERNEL
    assert kernels.count(want) == sum(o.builtin == B.BATCH_MATMUL for o in om.operators), kernels
    watch = list(ex.GetOutputs(key))
    if all_tensors:
        watch = [t.index for t in om.tensors if not t.is_const]
    views = {t: ex.GetTensorView(key, t) for t in watch}
    t_in = ex.GetInputs(key)[0]
    for i in range(3):
        ex.GetTensorView(key, t_in).GetData()[...] = xs[i]
        assert ex.ExecuteSubgraph(key).ok()
        for t, v in views.items():
            _compare(name, t, v.GetData(), refs_[i][t])


@pytest.mark.parametrize("name", ["attention_17_48_3", "attention_64_64_2", "vit_tiny_32", "const_rhs"])
def test_models_job_batches(gpu_lib, monkeypatch, model_refs, name):
    """the int8 models; an fp16-constant float model is not batchable whatever
    its ops (its DEQUANTIZE outputs have no unit batch dimension)"""
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf, xs, refs_ = model_refs[name]
    m, ex, key = _exec(buf, 73)
    st = ex.PrepareJobBatches(m, key, 5)
    assert st.ok(), st.message()
    assert ex.MaxJobBatch(key) == 5
    t_in = ex.GetInputs(key)[0]
    for n in (2, 3, 5):
        order = [(s + n) % 5 for s in range(n)]
        for s, i in enumerate(order):
            ex.GetJobSlotView(key, t_in, n, s).GetData()[...] = xs[i]
        for _ in range(2):
            assert ex.ExecuteJobBatch(key, n).ok()
            for s, i in enumerate(order):
                for t in ex.GetOutputs(key):
                    got = ex.GetJobSlotView(key, t, n, s).GetData()
                    _compare("%s n=%d slot %d" % (name, n, s), t, got.reshape(refs_[i][t].shape), refs_[i][t])


def test_rank2_model_runs_unbatched(gpu_lib, monkeypatch):
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf = B.rank2_model()
    m, ex, key = _exec(buf, 74)
    st = ex.PrepareJobBatches(m, key, 4)
    assert not st.ok() and "BATCH_MATMUL with a rank-2 activation operand" in st.message()
    assert ex.MaxJobBatch(key) == 1
    t_in, t_out = ex.GetInputs(key)[0], ex.GetOutputs(key)[0]
    for seed in (1, 2):
        x = R.zoo_input(buf, seed=seed)
        ref = run_reference(buf, x)
        ex.GetTensorView(key, t_in).GetData()[...] = x
        assert ex.ExecuteSubgraph(key).ok()
        np.testing.assert_array_equal(ex.GetTensorView(key, t_out).GetData().reshape(ref[t_out].shape), ref[t_out])


def test_engine_gpu_worker_only_serves_attention_block(gpu_lib, tmp_path, monkeypatch):
    """one Band engine whose only worker is a GPU worker registers the model -
    every op has to be in the kGPU set - and answers a request"""
    from band_amd.engine import Engine, JobStatus, Model, SchedulerType, make_config, kBandOk
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf = B.MODELS["attention_17_48_3"]()
    x = R.zoo_input(buf, seed=9)
    ref = run_reference(buf, x)
    outputs = OModel(buf).outputs
    e = Engine(make_config([SchedulerType.kRoundRobin], [DeviceFlag.kGPU]))
    path = str(tmp_path / "attention_block.tflite")
    with open(path, "wb") as f:
        f.write(buf)
    m = Model()
    assert m.FromPath(path)
    assert e.RegisterModel(m)
    assert e.GetNumOutputTensors(m) == len(outputs) == 1
    t = e.CreateInputTensor(m, 0)
    t.data()[...] = x
    outs = [e.CreateOutputTensor(m, 0)]
    h = e.RequestAsync(m, [t])
    assert h >= 0 and e.Wait(h, outs) == kBandOk
    assert e.GetJobRecord(h).status == JobStatus.kSuccess
    np.testing.assert_array_equal(outs[0].data().reshape(ref[outputs[0]].shape), ref[outputs[0]])
    e.close()
