"""The fused int8 attention launch on the MI355X: bh_attention_i8 on every case
of tests.attention_models.launcher_cases in both requantisation forms and on the
sum-order case (the kernel name is asserted first; the 0xff bytes around the
output must stay), what it refuses, and the models through the kGPU executor
with BAND_HIP_FUSED_ATTENTION=1 (eager, then replayed; one attention_i8_kernel
per attention and none of the launches it replaces; every tensor viewed: unfused
again; the flag unset or BAND_HIP_FUSION=0: the default launch list; job batches
2, 3, 5; an over-limit model), a GPU-only engine and the kCPU executor.

Reference: tests.attention_models (the oracle's FULLY_CONNECTED per batch slice
and the oracle's softmax) and run_reference for models; everything is compared with
assert_array_equal."""
import ctypes

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey
from oracle.tflite_fb import Model as OModel
from tests import attention_models as A
from tests import encoder_models as E
from tests.graph_reference import run_reference

pytestmark = pytest.mark.gpu

CASES = A.launcher_cases()
FLAG = "BAND_HIP_FUSED_ATTENTION"
REPLACED = ("bmm_mfma_kernel", "softmax_kernel")


@pytest.fixture(scope="module")
def refs():
    return {c.name: c.ref() for c in CASES}


@pytest.mark.parametrize("fast", [0, 1], ids=["two_step", "single_step"])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_attention_launcher(gpu_lib, refs, case, fast):
    """fast = 1 asks for the single-step requantisation of both products; the launcher takes it per product where
    bh_conv_requant_fast_ok holds"""
    np.testing.assert_array_equal(A.launch(case, gpu_lib, requant_fast=fast), refs[case.name], err_msg=case.name)


def test_launcher_decides_the_form_itself(gpu_lib, refs):
    for name in ("clamps", "qk_left_shift", "pv_left_shift", "batch_2x3_heads"):
        case = next(c for c in CASES if c.name == name)
        np.testing.assert_array_equal(A.launch(case, gpu_lib, requant_fast=-1), refs[name], err_msg=name)


def test_sum_order_case(gpu_lib):
    """the rows of tests/test_attention_cpu.py whose bytes change when the softmax's row sum is reversed or pairwise"""
    case, rev_rows, pair_rows = A.sum_order()
    assert case.keys == 196 and len(rev_rows) > 0 and len(pair_rows) > 0
    np.testing.assert_array_equal(A.launch(case, gpu_lib), case.ref())


@pytest.mark.parametrize("name,change,reason", A.refused_params(), ids=[r[0] for r in A.refused_params()])
def test_attention_refuses_bad_parameters(gpu_lib, name, change, reason):
    p, bufs, read = A.prepare(A.valid_case(), device=True)
    assert gpu_lib.bh_attention_i8_kernel(ctypes.byref(p)) == A.KERNEL.encode()
    change(p)
    assert gpu_lib.bh_attention_i8_kernel(ctypes.byref(p)) == b""
    assert gpu_lib.bh_attention_i8(ctypes.byref(p), None) != 0
    msg = gpu_lib.bh_last_error().decode()
    assert msg.startswith("bh_attention_i8: ") and reason in msg, msg
    assert gpu_lib.bh_attention_i8(None, None) != 0
    assert (bufs[3].download(np.uint8, (bufs[3].nbytes,)) == 0xff).all()


# ---- models --------------------------------------------------------------------------------
def _exec(buf, mid, flag=DeviceFlag.kGPU):
    m = HipModel(mid)
    assert m.FromBuffer(buf).ok()
    ex = HipModelExecutor(mid, 1, flag)
    assert ex.InvestigateModelSpec(m).unsupported_ops[flag] == set()
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    ex._model_ref = m
    return m, ex, SubgraphKey(mid, 1)


@pytest.fixture(scope="module")
def model_refs():
    out = {}
    for name, build in A.MODELS.items():
        buf = build()
        xs = [E.model_input(buf, seed=70 + i) for i in range(5)]
        out[name] = (buf, xs, [run_reference(buf, x) for x in xs])
    return out


def _kernels(ex, key):
    return [r["kernel"] for r in ex.ProfileSubgraph(key, iters=1)]


def _check_fused(name, kernels):
    assert kernels.count(A.KERNEL) == A.ATTENTIONS[name], kernels
    assert not [k for k in kernels if k in REPLACED or k.startswith("reindex")], kernels


@pytest.mark.parametrize("name", sorted(A.MODELS))
def test_models_fused(gpu_lib, monkeypatch, model_refs, name):
    """an eager pass, then the captured graph twice: one attention_i8_kernel per attention, no bmm_mfma_kernel,
    softmax_kernel or head-TRANSPOSE reindex launch; then every tensor viewed: the subgraph re-lowers unfused and
    every tensor (scores, probabilities, transposed heads included) is right"""
    monkeypatch.setenv(FLAG, "1")
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf, xs, refs_ = model_refs[name]
    m, ex, key = _exec(buf, 91)
    om = OModel(buf)
    _check_fused(name, _kernels(ex, key))
    t_in = ex.GetInputs(key)[0]
    for i in range(3):
        ex.GetTensorView(key, t_in).GetData()[...] = xs[i]
        assert ex.ExecuteSubgraph(key).ok()
        for t in ex.GetOutputs(key):
            np.testing.assert_array_equal(ex.GetTensorView(key, t).GetData().reshape(refs_[i][t].shape), refs_[i][t],
                                          err_msg="%s tensor %d pass %d" % (name, t, i))
    views = {t.index: ex.GetTensorView(key, t.index) for t in om.tensors if not t.is_const}
    kernels = _kernels(ex, key)
    assert A.KERNEL not in kernels and kernels.count("bmm_mfma_kernel") == 2 * A.ATTENTIONS[name], kernels
    assert kernels.count("softmax_kernel") == A.ATTENTIONS[name], kernels
    for i in range(3, 5):
        ex.GetTensorView(key, t_in).GetData()[...] = xs[i]
        assert ex.ExecuteSubgraph(key).ok()
        for t, v in views.items():
            np.testing.assert_array_equal(v.GetData().reshape(refs_[i][t].shape), refs_[i][t],
                                          err_msg="%s tensor %d" % (name, t))


def test_a_view_of_one_head_transpose_keeps_that_operand_dense(gpu_lib, monkeypatch, model_refs):
    """the transposed q viewed: its TRANSPOSE launch stays, the attention is still one launch"""
    monkeypatch.setenv(FLAG, "1")
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    name = "attention_17_48_3"
    buf, xs, refs_ = model_refs[name]
    m, ex, key = _exec(buf, 92)
    om = OModel(buf)
    (sc, pr, ctx), = A.attention_tensors(buf)
    tq = next(o for o in om.operators if o.outputs[0] == sc).inputs[0]
    view = ex.GetTensorView(key, tq)
    kernels = _kernels(ex, key)
    assert kernels.count(A.KERNEL) == 1 and len([k for k in kernels if k.startswith("reindex")]) == 1, kernels
    assert not [k for k in kernels if k in REPLACED], kernels
    t_in, t_out = ex.GetInputs(key)[0], ex.GetOutputs(key)[0]
    for i in range(2):
        ex.GetTensorView(key, t_in).GetData()[...] = xs[i]
        assert ex.ExecuteSubgraph(key).ok()
        np.testing.assert_array_equal(view.GetData().reshape(refs_[i][tq].shape), refs_[i][tq])
        np.testing.assert_array_equal(ex.GetTensorView(key, t_out).GetData().reshape(refs_[i][t_out].shape), refs_[i][t_out])


@pytest.mark.parametrize("env", [{}, {FLAG: "0"}, {FLAG: "1", "BAND_HIP_FUSION": "0"}], ids=["unset", "flag_0", "fusion_0"])
def test_switches_leave_the_default_launches(gpu_lib, monkeypatch, model_refs, env):
    monkeypatch.delenv(FLAG, raising=False)
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    buf, xs, refs_ = model_refs["attention_17_48_3"]
    m, ex, key = _exec(buf, 93)
    kernels = _kernels(ex, key)
    assert A.KERNEL not in kernels and kernels.count("bmm_mfma_kernel") == 2 and kernels.count("softmax_kernel") == 1
    assert len([k for k in kernels if k.startswith("reindex")]) == 4, kernels
    t_in, t_out = ex.GetInputs(key)[0], ex.GetOutputs(key)[0]
    ex.GetTensorView(key, t_in).GetData()[...] = xs[0]
    assert ex.ExecuteSubgraph(key).ok()
    np.testing.assert_array_equal(ex.GetTensorView(key, t_out).GetData().reshape(refs_[0][t_out].shape), refs_[0][t_out])


@pytest.mark.parametrize("name", ["attention_17_48_3", "encoder_17_48_3_96", "vit_tiny_32"])
def test_models_job_batches(gpu_lib, monkeypatch, model_refs, name):
    monkeypatch.setenv(FLAG, "1")
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf, xs, refs_ = model_refs[name]
    m, ex, key = _exec(buf, 94)
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
                    np.testing.assert_array_equal(got.reshape(refs_[i][t].shape), refs_[i][t],
                                                  err_msg="%s n=%d slot %d" % (name, n, s))


def test_over_limit_model_stays_unfused(gpu_lib, monkeypatch):
    """keys 1,025: the launcher's check refuses, the three launches stay and the model runs"""
    monkeypatch.setenv(FLAG, "1")
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf = A.shared_operand_model(1025)
    x = E.model_input(buf, seed=4)
    ref = run_reference(buf, x)
    m, ex, key = _exec(buf, 95)
    kernels = _kernels(ex, key)
    assert kernels == ["bmm_mfma_kernel", "softmax_kernel", "bmm_mfma_kernel"], kernels
    t_in, t_out = ex.GetInputs(key)[0], ex.GetOutputs(key)[0]
    for _ in range(2):
        ex.GetTensorView(key, t_in).GetData()[...] = x
        assert ex.ExecuteSubgraph(key).ok()
        np.testing.assert_array_equal(ex.GetTensorView(key, t_out).GetData().reshape(ref[t_out].shape), ref[t_out])


def test_cpu_executor_with_the_flag_gives_the_same_bytes(gpu_lib, monkeypatch, model_refs):
    monkeypatch.setenv(FLAG, "1")
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf, xs, refs_ = model_refs["attention_64_64_2"]
    m, ex, key = _exec(buf, 96, DeviceFlag.kCPU)
    assert A.KERNEL not in ex.LaunchKernels(key)
    mg, exg, keyg = _exec(buf, 97)
    _check_fused("attention_64_64_2", _kernels(exg, keyg))
    for e, k in ((ex, key), (exg, keyg)):
        e.GetTensorView(k, e.GetInputs(k)[0]).GetData()[...] = xs[0]
        assert e.ExecuteSubgraph(k).ok()
    t = ex.GetOutputs(key)[0]
    np.testing.assert_array_equal(ex.GetTensorView(key, t).GetData(), exg.GetTensorView(keyg, t).GetData())
    np.testing.assert_array_equal(ex.GetTensorView(key, t).GetData().reshape(refs_[0][t].shape), refs_[0][t])


def test_engine_gpu_worker_only_with_the_flag(gpu_lib, tmp_path, monkeypatch, model_refs):
    from band_amd.engine import Engine, JobStatus, Model, SchedulerType, make_config, kBandOk
    monkeypatch.setenv(FLAG, "1")
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf, xs, refs_ = model_refs["attention_17_48_3"]
    outputs = OModel(buf).outputs
    e = Engine(make_config([SchedulerType.kRoundRobin], [DeviceFlag.kGPU]))
    path = str(tmp_path / "attention_block.tflite")
    with open(path, "wb") as f:
        f.write(buf)
    m = Model()
    assert m.FromPath(path)
    assert e.RegisterModel(m)
    t = e.CreateInputTensor(m, 0)
    t.data()[...] = xs[0]
    outs = [e.CreateOutputTensor(m, 0)]
    h = e.RequestAsync(m, [t])
    assert h >= 0 and e.Wait(h, outs) == kBandOk
    assert e.GetJobRecord(h).status == JobStatus.kSuccess
    np.testing.assert_array_equal(outs[0].data().reshape(refs_[0][outputs[0]].shape), refs_[0][outputs[0]])
    e.close()
