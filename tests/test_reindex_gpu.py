"""The re-indexing ops on the MI355X: the bh_reindex launcher on every case of
tests.reindex_models.launcher_cases (rows, tile and gather paths), and the
model zoo through the kGPU executor (eager and replayed, every tensor viewed
and outputs only, job batches) and the engine.

Reference: numpy (the contiguous copy of the view a case is made of), and
tests.graph_reference.run_reference for models.  Integer tensors are compared
with assert_array_equal, float tensors at the tolerance of
tests/test_float_cpu.py."""
import ctypes

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey
from oracle.tflite_fb import Model as OModel
from tests import reindex_models as R
from tests.graph_reference import run_reference
from tests.test_float_cpu import assert_float_close

pytestmark = pytest.mark.gpu

CASES = [(name, dt, shape, view, kernel, mis) for name, dts, shape, view, kernel, mis in R.launcher_cases()
         for dt in dts]


def _launch(lib, x, v, misalign=0):
    """bh_reindex of the view v of x; the input sits `misalign` bytes into its
    buffer, the output buffer is 0xff and 16 bytes longer than the result"""
    from band_amd import _abi
    from band_amd.device import DeviceBuffer
    want = np.ascontiguousarray(v)
    raw = np.concatenate([np.zeros(misalign, np.uint8), x.view(np.uint8).reshape(-1)])
    dx = DeviceBuffer.from_array(raw)
    dy = DeviceBuffer.from_array(np.full(want.nbytes + 16, 0xff, np.uint8))
    p = R.reindex_params(x, v, dx.value + misalign, dy.value)
    kernel = lib.bh_reindex_kernel(ctypes.byref(p)).decode()
    _abi.check(lib.bh_reindex(ctypes.byref(p), None), "bh_reindex")
    got = dy.download(np.uint8, want.nbytes + 16)
    assert (got[want.nbytes:] == 0xff).all(), "bytes past the output were written"
    return got[:want.nbytes].view(x.dtype).reshape(want.shape), want, kernel


@pytest.mark.parametrize("name,dtype,shape,view,kernel,misalign", CASES,
                         ids=["%s-%s" % (c[0], np.dtype(c[1]).name) for c in CASES])
def test_reindex_launcher(gpu_lib, name, dtype, shape, view, kernel, misalign):
    x = R.fill(shape, dtype)
    got, want, ran = _launch(gpu_lib, x, view(x), misalign)
    if kernel is not None:
        assert ran == kernel
    np.testing.assert_array_equal(got, want, err_msg=ran)


def test_reindex_refuses_bad_parameters(gpu_lib):
    from band_amd import _abi
    from band_amd.device import DeviceBuffer
    dx, dy = DeviceBuffer(256), DeviceBuffer(256)
    ok = dict(elem_bytes=4, rank=2, in_offset=0, input=dx.value, output=dy.value)
    for bad in (dict(rank=7), dict(elem_bytes=2), dict(input=dx.value + 2), dict(output=None), dict(rank=-1)):
        kw = dict(ok)
        kw.update(bad)
        p = _abi.ReindexParams(**kw)
        for d in range(min(max(p.rank, 0), 6)):
            p.out_dims[d], p.in_stride[d] = 2, 1
        assert gpu_lib.bh_reindex(ctypes.byref(p), None) != 0
        assert b"bh_reindex" in gpu_lib.bh_last_error()
    p = _abi.ReindexParams(**ok)  # 2^31 elements
    p.out_dims[0], p.out_dims[1], p.in_stride[0], p.in_stride[1] = 1 << 16, 1 << 15, 0, 0
    assert gpu_lib.bh_reindex(ctypes.byref(p), None) != 0 and b"2^31" in gpu_lib.bh_last_error()


# ---- models --------------------------------------------------------------------------
def _exec(buf, mid):
    m = HipModel(mid)
    assert m.FromBuffer(buf).ok()
    ex = HipModelExecutor(mid, 1, DeviceFlag.kGPU)
    assert ex.InvestigateModelSpec(m).unsupported_ops[DeviceFlag.kGPU] == set()
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
def zoo_refs():
    """per model: its bytes, 5 inputs and run_reference of each"""
    out = {}
    for name, build in R.ZOO.items():
        buf = build()
        xs = [R.zoo_input(buf, seed=20 + i) for i in range(5)]
        out[name] = (buf, xs, [run_reference(buf, x) for x in xs])
    return out


@pytest.mark.parametrize("all_tensors", [False, True], ids=["outputs", "every_tensor"])
@pytest.mark.parametrize("name", sorted(R.ZOO))
def test_zoo_gpu_executor(gpu_lib, monkeypatch, zoo_refs, name, all_tensors):
    """an eager pass, then the captured graph twice; with only the outputs
    viewed (the fusions stand) and with every non-constant tensor viewed"""
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf, xs, refs = zoo_refs[name]
    m, ex, key = _exec(buf, 61)
    om = OModel(buf)
    kernels = [r["kernel"] for r in ex.ProfileSubgraph(key, iters=1)]
    assert any(k.startswith("reindex_") for k in kernels), kernels
    watch = list(ex.GetOutputs(key))
    if all_tensors:
        watch = [t.index for t in om.tensors if not t.is_const]
    views = {t: ex.GetTensorView(key, t) for t in watch}
    t_in = ex.GetInputs(key)[0]
    for i in range(3):
        ex.GetTensorView(key, t_in).GetData()[...] = xs[i]
        assert ex.ExecuteSubgraph(key).ok()
        for t, v in views.items():
            _compare(name, t, v.GetData(), refs[i][t])


def test_zoo_kernels(gpu_lib, monkeypatch):
    """the zoo's launches, by kernel: the channel split, the depth / space ops
    and the head's transpose and box / class slices (channels stay innermost)
    are rows; its one-channel objectness slice (unit rows at stride 9) and the
    channel shuffle (a 16 x 2 transpose, too short for a tile) are gathers"""
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    for name, want in (("shuffle_unit", {"reindex_rows_kernel", "reindex_gather_kernel"}),
                       ("detector_head_i8", {"reindex_rows_kernel", "reindex_gather_kernel"}),
                       ("subpixel", {"reindex_rows_kernel"})):
        m, ex, key = _exec(R.ZOO[name](), 62)
        got = {r["kernel"] for r in ex.ProfileSubgraph(key, iters=1) if r["kernel"].startswith("reindex_")}
        assert got == want, (name, got)


@pytest.mark.parametrize("name", ["shuffle_unit", "subpixel"])
def test_zoo_job_batches(gpu_lib, monkeypatch, zoo_refs, name):
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf, xs, refs = zoo_refs[name]
    m, ex, key = _exec(buf, 63)
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
                    _compare("%s n=%d slot %d" % (name, n, s), t, got.reshape(refs[i][t].shape), refs[i][t])


def test_batch_axis_transpose_runs_unbatched(gpu_lib, monkeypatch):
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf = R.batch_axis_transpose()
    m, ex, key = _exec(buf, 64)
    st = ex.PrepareJobBatches(m, key, 4)
    assert not st.ok() and "TRANSPOSE does not keep the whole batch axis" in st.message()
    assert ex.MaxJobBatch(key) == 1
    t_in, t_out = ex.GetInputs(key)[0], ex.GetOutputs(key)[0]
    for seed in (1, 2):
        x = R.zoo_input(buf, seed=seed)
        ref = run_reference(buf, x)
        ex.GetTensorView(key, t_in).GetData()[...] = x
        assert ex.ExecuteSubgraph(key).ok()
        np.testing.assert_array_equal(ex.GetTensorView(key, t_out).GetData().reshape(ref[t_out].shape), ref[t_out])


def test_engine_gpu_worker_only_serves_detector_head(gpu_lib, tmp_path, monkeypatch):
    """one Band engine whose only worker is a GPU worker registers the model -
    every op has to be in the kGPU set - and answers a request"""
    from band_amd.engine import Engine, JobStatus, Model, SchedulerType, make_config, kBandOk
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf = R.detector_head(np.int8)
    x = R.zoo_input(buf, seed=9)
    ref = run_reference(buf, x)
    outputs = OModel(buf).outputs
    e = Engine(make_config([SchedulerType.kRoundRobin], [DeviceFlag.kGPU]))
    path = str(tmp_path / "detector_head.tflite")
    with open(path, "wb") as f:
        f.write(buf)
    m = Model()
    assert m.FromPath(path)
    assert e.RegisterModel(m)
    assert e.GetNumOutputTensors(m) == len(outputs) == 3
    t = e.CreateInputTensor(m, 0)
    t.data()[...] = x
    outs = [e.CreateOutputTensor(m, k) for k in range(3)]
    h = e.RequestAsync(m, [t])
    assert h >= 0 and e.Wait(h, outs) == kBandOk
    assert e.GetJobRecord(h).status == JobStatus.kSuccess
    for k, o in enumerate(outs):
        np.testing.assert_array_equal(o.data().reshape(ref[outputs[k]].shape), ref[outputs[k]])
    e.close()
