"""CAST and the padded text models on the MI355X: cast_kernel on all 16 type
pairs at counts 1, 63, 64, 65 and 4,099 with the pointers on their buffers, 4
bytes off and (the uint8 side) 1 byte off, into 0xff buffers whose surroundings
must stay; one-op CAST models; text_encoder(mask=True, pooler=True,
embedding_lookup=True) as int8 / float32 / hybrid through the kGPU executor
with BAND_HIP_FUSED_ATTENTION unset and set (eager, then replayed; with the flag
one attention_bias_i8_kernel per block of the int8 model and none of the
launches it replaces), job batches 2, 3 and 5, a GPU-only engine, and the exact
masked-ids test on the float32 model.

References: tests.cast_models (numpy and Python integers) and run_reference."""
import ctypes

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey, _abi
from oracle.tflite_fb import Model as OModel
from tests import cast_models as C
from tests import mask_models as M
from tests.graph_reference import run_reference
from tests.test_float_cpu import assert_float_close

pytestmark = pytest.mark.gpu

PAIRS = [(a, b) for a in C.TYPES for b in C.TYPES]
PAIR_IDS = ["%s_to_%s" % (np.dtype(a).name, np.dtype(b).name) for a, b in PAIRS]
FLAG = "BAND_HIP_FUSED_ATTENTION"
GUARD = 32


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_cast_kernel_every_pair(gpu_lib, pair):
    from band_amd.device import DeviceBuffer
    src_t, dst_t = pair
    s1, d1 = np.dtype(src_t).itemsize == 1, np.dtype(dst_t).itemsize == 1
    offsets = [(0, 0), (4, 4), (4, 0), (0, 4)] + ([(1, 0)] if s1 else []) + ([(0, 1)] if d1 else []) + ([(1, 1)] if s1 and d1 else [])
    for count in C.COUNTS:
        x = C.source(src_t, count)
        want = C.cast_ref(x, dst_t)
        for so, do in offsets:
            din = DeviceBuffer.from_array(np.concatenate([np.zeros(so, np.uint8), x.view(np.uint8)]))
            dout = DeviceBuffer.from_array(np.full(GUARD + do + want.nbytes + GUARD, 0xff, np.uint8))
            p = _abi.CastParams(C.CODE[np.dtype(src_t)], C.CODE[np.dtype(dst_t)], count, din.value + so,
                                dout.value + GUARD + do)
            _abi.check(gpu_lib.bh_cast(ctypes.byref(p), None), "bh_cast")
            raw = dout.download(np.uint8, (GUARD + do + want.nbytes + GUARD,))
            got = raw[GUARD + do:GUARD + do + want.nbytes].copy().view(dst_t)
            assert got.tobytes() == want.tobytes(), (count, so, do, x[got != want][:5], got[got != want][:5], want[got != want][:5])
            assert (raw[:GUARD + do] == 0xff).all() and (raw[GUARD + do + want.nbytes:] == 0xff).all(), (count, so, do)
            din.free()
            dout.free()


def test_cast_refuses_a_misaligned_float_pointer(gpu_lib):
    from band_amd.device import DeviceBuffer
    d = DeviceBuffer(64)
    o = DeviceBuffer(64)
    p = _abi.CastParams(4, 2, 8, d.value + 1, o.value)
    assert gpu_lib.bh_cast(ctypes.byref(p), None) != 0 and b"not aligned" in gpu_lib.bh_last_error()


def _exec(buf, mid, flag=DeviceFlag.kGPU):
    m = HipModel(mid)
    assert m.FromBuffer(buf).ok()
    ex = HipModelExecutor(mid, 1, flag)
    assert ex.InvestigateModelSpec(m).unsupported_ops[flag] == set()
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    ex._model_ref = m
    return m, ex, SubgraphKey(mid, 1)


@pytest.mark.parametrize("pair", [(np.int32, np.float32), (np.float32, np.int64), (np.int64, np.uint8), (np.uint8, np.uint8)],
                         ids=["i32_f32", "f32_i64", "i64_u8", "u8_u8"])
def test_one_cast_models(gpu_lib, pair):
    src_t, dst_t = pair
    x = C.source(src_t, 65).reshape(1, 5, 13)
    m, ex, key = _exec(C.raw_cast((1, 5, 13), src_t, dst_t), 50)
    assert ex.LaunchKernels(key) == (["copy"] if src_t == dst_t else ["cast_kernel"])
    ex.GetTensorView(key, ex.GetInputs(key)[0]).GetData()[...] = x
    for _ in range(2):  # eager, then the captured graph
        assert ex.ExecuteSubgraph(key).ok()
        assert ex.GetTensorView(key, ex.GetOutputs(key)[0]).GetData().tobytes() == C.cast_ref(x, dst_t).tobytes()


def _compare(name, t, got, ref):
    assert got.dtype == ref.dtype, (name, t)
    if ref.dtype == np.float32:
        assert_float_close(got, ref, "%s tensor %d" % (name, t))
    else:
        np.testing.assert_array_equal(got.reshape(ref.shape), ref, err_msg="%s tensor %d" % (name, t))


@pytest.fixture(scope="module")
def model_refs():
    out = {}
    for name, build in C.PADDED.items():
        for batch in (2, 1):
            buf = build(batch=batch)
            xs = [C.inputs(buf, seed=s) for s in range(3)]
            out[name, batch] = (buf, xs, [run_reference(buf, x, table=C.REF_TABLE) for x in xs])
    return out


@pytest.mark.parametrize("fused", [False, True], ids=["flag_unset", "flag_set"])
@pytest.mark.parametrize("all_tensors", [False, True], ids=["outputs", "every_tensor"])
@pytest.mark.parametrize("name", sorted(C.PADDED))
def test_padded_text_models_gpu_executor(gpu_lib, monkeypatch, model_refs, name, all_tensors, fused):
    for v in ("BAND_HIP_FUSION", FLAG, "BAND_HIP_FUSED_LAYERNORM_F32"):
        monkeypatch.delenv(v, raising=False)
    if fused:
        monkeypatch.setenv(FLAG, "1")
    buf, xs, refs = model_refs[name, 2]
    m, ex, key = _exec(buf, 51)
    om = OModel(buf)
    watch = [t.index for t in om.tensors if not t.is_const] if all_tensors else list(ex.GetOutputs(key))
    views = {t: ex.GetTensorView(key, t) for t in watch}
    kernels = ex.LaunchKernels(key)
    assert kernels.count("cast_kernel") == 1, kernels
    if name.endswith("i8") and fused and not all_tensors:
        # per block: one masked fused launch, none of the launches it replaces, the LayerNorms still fire
        assert kernels.count(M.KERNEL) == 2 and "attention_i8_kernel" not in kernels, kernels
        assert not [k for k in kernels if k in ("bmm_mfma_kernel", "softmax_kernel")], kernels
        # no head TRANSPOSE launch: the one re-indexing launch left is the STRIDED_SLICE of token 0
        assert len([k for k in kernels if k.startswith("reindex")]) == 1, kernels
        assert kernels.count("layernorm_i8_kernel") == 5, kernels
    else:
        assert M.KERNEL not in kernels
    if name.endswith("i8") and not fused:
        assert kernels.count("bmm_mfma_kernel") == 4 and kernels.count("softmax_kernel") == 2, kernels
    for i in range(3):
        for t, v in xs[i].items():
            ex.GetTensorView(key, t).GetData()[...] = v
        assert ex.ExecuteSubgraph(key).ok()
        for t, v in views.items():
            _compare(name, t, v.GetData(), refs[i][t])


@pytest.mark.parametrize("name", ["padded_text_i8", "padded_text_hybrid"])
def test_padded_text_models_job_batches(gpu_lib, monkeypatch, model_refs, name):
    """job batches 2, 3 and 5 against the reference of each job's own inputs; the mask's axis 0 is the job axis, and
    with the flag every variant of the int8 model keeps one masked fused launch per block"""
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    monkeypatch.setenv(FLAG, "1")
    buf, xs, refs = model_refs[name, 1]
    m, ex, key = _exec(buf, 52)
    st = ex.PrepareJobBatches(m, key, 5)
    assert st.ok(), st.message()
    for n in (2, 3, 5):
        if name.endswith("i8"):
            assert ex.JobBatchLaunchKernels(key, n).count(M.KERNEL) == 2
        order = [(s + n) % 3 for s in range(n)]
        for s, i in enumerate(order):
            for t, v in xs[i].items():
                ex.GetJobSlotView(key, t, n, s).GetData()[...] = v
        for _ in range(2):
            assert ex.ExecuteJobBatch(key, n).ok()
            for s, i in enumerate(order):
                for t in ex.GetOutputs(key):
                    _compare(name, t, ex.GetJobSlotView(key, t, n, s).GetData().reshape(refs[i][t].shape), refs[i][t])


def test_engine_gpu_worker_serves_the_padded_text_encoder(gpu_lib, tmp_path, monkeypatch, model_refs):
    from band_amd.engine import Engine, JobStatus, Model, SchedulerType, make_config, kBandOk
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    monkeypatch.setenv(FLAG, "1")
    buf, xs, refs = model_refs["padded_text_i8", 1]
    om = OModel(buf)
    e = Engine(make_config([SchedulerType.kRoundRobin], [DeviceFlag.kGPU]))
    path = str(tmp_path / "padded_text.tflite")
    with open(path, "wb") as f:
        f.write(buf)
    m = Model()
    assert m.FromPath(path)
    assert e.RegisterModel(m)
    for i in range(2):
        ins = []
        for k, t in enumerate(om.inputs):
            ten = e.CreateInputTensor(m, k)
            ten.data()[...] = xs[i][t]
            ins.append(ten)
        outs = [e.CreateOutputTensor(m, 0)]
        h = e.RequestAsync(m, ins)
        assert h >= 0 and e.Wait(h, outs) == kBandOk
        assert e.GetJobRecord(h).status == JobStatus.kSuccess
        np.testing.assert_array_equal(outs[0].data().reshape(refs[i][om.outputs[0]].shape), refs[i][om.outputs[0]])
    e.close()


def test_masked_ids_leave_the_logits_alone_on_the_gpu(gpu_lib, monkeypatch):
    from tests.test_cast_mask_cpu import masked_ids_leave_the_logits_alone
    for v in ("BAND_HIP_FUSION", FLAG, "BAND_HIP_FUSED_LAYERNORM_F32"):
        monkeypatch.delenv(v, raising=False)
    masked_ids_leave_the_logits_alone(DeviceFlag.kGPU, 1)
