"""TANH and EMBEDDING_LOOKUP on the MI355X (CAST and the padded text models: tests/test_cast_mask_*.py): the 8-bit TANH
as a one-op model over all 256 bytes, bh_unary_f32's BH_UNARY_TANH against
float64 tanh at the device library's bound, EMBEDDING_LOOKUP through
tests.gather_models' axis-0 cases as one-op models, and the text models with a
pooler and an EMBEDDING_LOOKUP through the kGPU executor (eager, then replayed;
outputs and every tensor; job batches 2 and 3) and a GPU-only engine.

References: tests.tanh_lookup_models (numpy; libm's tanhf for the 8-bit table)
and run_reference with its table."""
import ctypes

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey, _abi
from oracle.tflite_fb import Model as OModel
from tests import gather_models as G
from tests import tanh_lookup_models as T
from tests.graph_reference import run_reference
from tests.test_float_cpu import assert_float_close

pytestmark = pytest.mark.gpu


def _exec(buf, mid, flag=DeviceFlag.kGPU):
    m = HipModel(mid)
    assert m.FromBuffer(buf).ok()
    ex = HipModelExecutor(mid, 1, flag)
    assert ex.InvestigateModelSpec(m).unsupported_ops[flag] == set()
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    ex._model_ref = m
    return m, ex, SubgraphKey(mid, 1)


def _run(buf, feeds, mid=60, passes=2):
    m, ex, key = _exec(buf, mid)
    for t, x in zip(ex.GetInputs(key), feeds):
        ex.GetTensorView(key, t).GetData()[...] = x
    for _ in range(passes):  # eager, then the captured graph
        assert ex.ExecuteSubgraph(key).ok()
    return [ex.GetTensorView(key, t).GetData().copy() for t in ex.GetOutputs(key)], ex.LaunchKernels(key)


@pytest.mark.parametrize("q", T.TANH_Q, ids=["%s_%g" % ("i8" if q[0] else "u8", q[1]) for q in T.TANH_Q])
def test_one_tanh_model_is_the_table(gpu_lib, q):
    signed, s_in, z_in, s_out, z_out = q
    dt = np.int8 if signed else np.uint8
    x = np.arange(256, dtype=np.uint8).view(dt).reshape(1, 4, 64)
    (got,), kernels = _run(T.raw_tanh((1, 4, 64), dt, in_q=(s_in, z_in), out_q=(s_out, z_out)), [x])
    assert kernels == ["lut_u8_kernel"]
    np.testing.assert_array_equal(got.reshape(-1).view(np.uint8), T.np_tanh_table(*q)[x.reshape(-1).view(np.uint8)])


def test_float32_tanh_kernel(gpu_lib):
    """|got - tanh(x)| <= gamma(k) |y| + 2^-126 against float64 tanh, k = 32: the device library's tanhf at 16 ulp, as
    tests.float_harness takes it for GELU's tanh form, an ulp being at most 2 u |y|.  Observed on an MI355X: 0.070 of
    the bound at the worst input."""
    from band_amd.device import DeviceBuffer
    x = T.tanh_f32_inputs()
    dx, dy = DeviceBuffer.from_array(x), DeviceBuffer(x.nbytes)
    _abi.check(gpu_lib.bh_unary_f32(6, dx.value, dy.value, x.size, ctypes.c_float(0), ctypes.c_float(0), None), "unary")
    got = dy.download(np.float32, x.shape)
    ref = np.tanh(x.astype(np.float64))
    err = np.abs(got.astype(np.float64) - ref)
    tol = T.tanh_f32_bound(ref, "device")
    print("float32 TANH (device): largest |error| / bound %.3f" % (err / tol).max())
    assert (err <= tol).all()
    for kind in (5, 7):  # BH_UNARY_TANH is 6: 5 stays no kind
        assert gpu_lib.bh_unary_f32(kind, dx.value, dy.value, x.size, ctypes.c_float(0), ctypes.c_float(0), None) != 0


def test_one_float32_tanh_model(gpu_lib):
    x = T.tanh_f32_inputs()[:4096].reshape(1, 64, 64)
    (got,), kernels = _run(T.raw_tanh((1, 64, 64), np.float32, in_q=None, out_q=None), [x])
    assert kernels == ["unary_f32_kernel"]
    ref = np.tanh(x.astype(np.float64))
    assert (np.abs(got.reshape(ref.shape).astype(np.float64) - ref) <= T.tanh_f32_bound(ref, "device")).all()


AXIS0 = [c for c in G.launcher_cases() if c.axis == 0 and not c.int64_only and c.misalign == 0]


@pytest.mark.parametrize("case", AXIS0, ids=[c.name for c in AXIS0])
def test_embedding_lookup_on_the_gather_cases(gpu_lib, case):
    index_dtype = np.int64 if len(case.name) % 2 else np.int32
    buf = T.raw_lookup(case.shape, case.indices, case.dtype, index_dtype=index_dtype)
    (got,), kernels = _run(buf, [np.asarray(case.indices, index_dtype)])
    assert kernels == [G.KERNEL]
    np.testing.assert_array_equal(got.reshape(case.ref().shape), case.ref())


def _compare(name, t, got, ref):
    assert got.dtype == ref.dtype, (name, t)
    if ref.dtype == np.float32:
        assert_float_close(got, ref, "%s tensor %d" % (name, t))
    else:
        np.testing.assert_array_equal(got.reshape(ref.shape), ref, err_msg="%s tensor %d" % (name, t))


@pytest.fixture(scope="module")
def model_refs():
    out = {}
    for name, build in T.TEXT_MODELS.items():
        buf = build(batch=1)
        xs = [T.token_ids(buf, seed=s) for s in range(3)]
        out[name] = (buf, xs, [run_reference(buf, x, table=T.REF_TABLE) for x in xs])
    return out


@pytest.mark.parametrize("all_tensors", [False, True], ids=["outputs", "every_tensor"])
@pytest.mark.parametrize("name", sorted(T.TEXT_MODELS))
def test_text_models_gpu_executor(gpu_lib, monkeypatch, model_refs, name, all_tensors):
    for v in ("BAND_HIP_FUSION", "BAND_HIP_FUSED_ATTENTION", "BAND_HIP_FUSED_LAYERNORM_F32"):
        monkeypatch.delenv(v, raising=False)
    buf, xs, refs = model_refs[name]
    m, ex, key = _exec(buf, 61)
    om = OModel(buf)
    watch = [t.index for t in om.tensors if not t.is_const] if all_tensors else list(ex.GetOutputs(key))
    views = {t: ex.GetTensorView(key, t) for t in watch}
    kernels = ex.LaunchKernels(key)
    assert kernels[0] == G.KERNEL and kernels.count(G.KERNEL) == 1, kernels
    if not name.endswith("i8"):
        assert "unary_f32_kernel" in kernels
    elif all_tensors:  # (with the pooler's projection private, the 8-bit table folds into the launch before it)
        assert "lut_u8_kernel" in kernels
    t_in = ex.GetInputs(key)[0]
    for i in range(3):
        ex.GetTensorView(key, t_in).GetData()[...] = xs[i]
        assert ex.ExecuteSubgraph(key).ok()
        for t, v in views.items():
            _compare(name, t, v.GetData(), refs[i][t])


@pytest.mark.parametrize("name", ["text_pooler_i8", "text_pooler_hybrid"])
def test_text_models_job_batches(gpu_lib, monkeypatch, model_refs, name):
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf, xs, refs = model_refs[name]
    m, ex, key = _exec(buf, 62)
    st = ex.PrepareJobBatches(m, key, 3)
    assert st.ok(), st.message()
    t_in = ex.GetInputs(key)[0]
    for n in (2, 3):
        order = [(s + n) % 3 for s in range(n)]
        for s, i in enumerate(order):
            ex.GetJobSlotView(key, t_in, n, s).GetData()[...] = xs[i]
        for _ in range(2):
            assert ex.ExecuteJobBatch(key, n).ok()
            for s, i in enumerate(order):
                for t in ex.GetOutputs(key):
                    _compare(name, t, ex.GetJobSlotView(key, t, n, s).GetData().reshape(refs[i][t].shape), refs[i][t])


def test_engine_gpu_worker_serves_the_pooled_text_model(gpu_lib, tmp_path, model_refs):
    from band_amd.engine import Engine, JobStatus, Model, SchedulerType, make_config, kBandOk
    buf, xs, refs = model_refs["text_pooler_i8"]
    out_t = OModel(buf).outputs[0]
    e = Engine(make_config([SchedulerType.kRoundRobin], [DeviceFlag.kGPU]))
    path = str(tmp_path / "text_pooler.tflite")
    with open(path, "wb") as f:
        f.write(buf)
    m = Model()
    assert m.FromPath(path)
    assert e.RegisterModel(m)
    for i in range(2):
        t = e.CreateInputTensor(m, 0)
        t.data()[...] = xs[i]
        outs = [e.CreateOutputTensor(m, 0)]
        h = e.RequestAsync(m, [t])
        assert h >= 0 and e.Wait(h, outs) == kBandOk
        assert e.GetJobRecord(h).status == JobStatus.kSuccess
        np.testing.assert_array_equal(outs[0].data().reshape(refs[i][out_t].shape), refs[i][out_t])
    e.close()
