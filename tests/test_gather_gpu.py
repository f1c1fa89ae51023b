"""GATHER, PACK, UNPACK and TILE on the MI355X: the bh_gather launcher on the
case table of tests.gather_models (int32 and int64 indices, guarded and
poisoned outputs, the table between guard rows), its refusals, the TILE maps
on the kernels of reindex.hip, and text_encoder and the PACK / UNPACK / TILE
zoo through the kGPU executor (eager and replayed, every tensor viewed), job
batches, the engine and the two opt-in fusion flags.

Reference: numpy (tests/gather_models.py) and
tests.graph_reference.run_reference with the family's table entries.  Integer
tensors are compared with assert_array_equal, float tensors with
assert_float_close of tests/test_float_cpu.py.

Out-of-range indices here are only those whose unguarded address would still
fall inside the test's own buffer (the guard rows); the extreme values run on
the CPU through the range function the kernel shares (tests/test_gather_cpu.py)."""
import ctypes

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey, _abi
from oracle.tflite_fb import Model as OModel
from tests import gather_models as G
from tests.graph_reference import TABLE, run_reference
from tests.guarded_output import GuardedOutput
from tests.test_float_cpu import assert_float_close

pytestmark = pytest.mark.gpu

REF_TABLE = TABLE + G.ENTRIES
CASES = [(c, dt) for c in G.launcher_cases() for dt in (np.int32, np.int64) if dt == np.int64 or not c.int64_only]
IDS = ["%s-%s" % (c.name, np.dtype(dt).name) for c, dt in CASES]


# ---- the launcher ------------------------------------------------------------------------
@pytest.mark.parametrize("case,index_dtype", CASES, ids=IDS)
def test_gather_launcher(gpu_lib, case, index_dtype):
    from band_amd.device import DeviceBuffer
    outer, axis_size, inner = case.counts()
    row = inner * case.dtype.itemsize
    # no test index may leave the buffer even unguarded: at most GUARD_ROWS rows past either end
    # (the int64 values narrow to rows inside the table)
    for v in case.indices:
        assert -G.GUARD_ROWS <= v < axis_size + G.GUARD_ROWS or (case.int64_only and 0 <= v % 2**32 < axis_size)
    want = case.ref()
    raw, at = case.guarded_table()
    assert at >= G.GUARD_ROWS * row and raw.size - at - outer * axis_size * row >= G.GUARD_ROWS * row
    table = DeviceBuffer.from_array(raw)
    idx = DeviceBuffer.from_array(np.asarray(case.indices, index_dtype))
    out = GuardedOutput(want.nbytes, expect=want)
    p = G.gather_params(case, index_dtype, table.value + at, idx.value, out.value)
    assert (table.value + at) % 16 == case.misalign
    assert gpu_lib.bh_gather_kernel(ctypes.byref(p)).decode() == G.KERNEL
    _abi.check(gpu_lib.bh_gather(ctypes.byref(p), None), "bh_gather")
    got = out.download(case.dtype, want.shape)
    np.testing.assert_array_equal(got, want, err_msg=case.name)
    for b in (table, idx):
        b.free()
    out.free()


@pytest.mark.parametrize("name", ["outer3_axis1_float32", "out_of_range_u8", "u8_row1040"])
def test_a_map_with_indices_through_bh_reindex(gpu_lib, name):
    """what the executor launches: bh_reindex on a map that carries the index tensor"""
    from band_amd.device import DeviceBuffer
    case = next(c for c in G.launcher_cases() if c.name == name)
    want = case.ref()
    raw, at = case.guarded_table()
    table = DeviceBuffer.from_array(raw)
    idx = DeviceBuffer.from_array(np.asarray(case.indices, np.int32))
    out = GuardedOutput(want.nbytes, expect=want)
    p = G.indexed_map(case, np.int32, table.value + at, idx.value, out.value)
    assert gpu_lib.bh_reindex_kernel(ctypes.byref(p)).decode() == G.KERNEL
    _abi.check(gpu_lib.bh_reindex(ctypes.byref(p), None), "bh_reindex")
    np.testing.assert_array_equal(out.download(case.dtype, want.shape), want, err_msg=name)
    p.in_offset = 1
    assert gpu_lib.bh_reindex(ctypes.byref(p), None) != 0 and b"a map with indices" in gpu_lib.bh_last_error()
    assert gpu_lib.bh_reindex_as(ctypes.byref(p), 1, None) != 0
    for b in (table, idx):
        b.free()
    out.free()


def test_gather_refuses_bad_parameters(gpu_lib):
    from band_amd.device import DeviceBuffer
    dx, di, dy = DeviceBuffer(256), DeviceBuffer(256), DeviceBuffer.from_array(np.full(256, 0xff, np.uint8))
    ok = dict(elem_bytes=4, index_bytes=4, outer=1, axis_size=4, n_idx=2, inner=4, params=dx.value, indices=di.value,
              output=dy.value)
    for bad in (dict(params=None), dict(indices=None), dict(output=None), dict(elem_bytes=2), dict(index_bytes=2),
                dict(params=dx.value + 2), dict(output=dy.value + 2), dict(n_idx=1 << 20, inner=1 << 9)):
        p = _abi.GatherParams(**dict(ok, **bad))
        assert gpu_lib.bh_gather(ctypes.byref(p), None) != 0
        assert gpu_lib.bh_last_error().startswith(b"bh_gather: "), gpu_lib.bh_last_error()
        assert gpu_lib.bh_gather_kernel(ctypes.byref(p)) == b""
    assert b"2^31" in gpu_lib.bh_last_error()
    assert gpu_lib.bh_gather(None, None) != 0 and b"bh_gather" in gpu_lib.bh_last_error()
    assert (dy.download(np.uint8, (256,)) == 0xff).all()


@pytest.mark.parametrize("name,shape,multiples,kernel", G.TILE_MAPS, ids=[t[0] for t in G.TILE_MAPS])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_tile_maps_on_the_reindex_kernels(gpu_lib, name, shape, multiples, kernel, dtype):
    """a zero input stride through reindex_rows_kernel, reindex_gather_kernel and reindex_tile_kernel"""
    from band_amd.device import DeviceBuffer
    x = G.fill(shape, dtype)
    want = np.ascontiguousarray(np.tile(x, multiples))
    dx = DeviceBuffer.from_array(x.reshape(-1).view(np.uint8))
    out = GuardedOutput(want.nbytes, expect=want)
    p = G.tile_map(shape, multiples, dtype, dx.value, out.value)
    assert gpu_lib.bh_reindex_kernel(ctypes.byref(p)).decode() == kernel
    _abi.check(gpu_lib.bh_reindex(ctypes.byref(p), None), "bh_reindex")
    np.testing.assert_array_equal(out.download(dtype, want.shape), want, err_msg=name)
    dx.free()
    out.free()


# ---- models --------------------------------------------------------------------------------
def _exec(buf, mid, flag=DeviceFlag.kGPU):
    m = HipModel(mid)
    assert m.FromBuffer(buf).ok()
    ex = HipModelExecutor(mid, 1, flag)
    spec = ex.InvestigateModelSpec(m)
    assert spec.unsupported_ops[DeviceFlag.kGPU] == set() and spec.unsupported_ops[DeviceFlag.kCPU] == set()
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


def _input(name, buf, seed):
    return G.token_ids(buf, seed) if name in G.TEXT_ENCODERS else G.zoo_input(buf, seed)


@pytest.fixture(scope="module")
def model_refs():
    """per model: its bytes, 3 inputs and run_reference of each"""
    out = {}
    for name, build in list(G.TEXT_ENCODERS.items()) + list(G.ZOO.items()):
        buf = build()
        xs = [_input(name, buf, 20 + i) for i in range(3)]
        out[name] = (buf, xs, [run_reference(buf, x, table=REF_TABLE) for x in xs])
    return out


@pytest.mark.parametrize("all_tensors", [False, True], ids=["outputs", "every_tensor"])
@pytest.mark.parametrize("name", sorted(G.TEXT_ENCODERS) + sorted(G.ZOO))
def test_models_gpu_executor(gpu_lib, monkeypatch, model_refs, name, all_tensors):
    """an eager pass, then the captured graph twice; with only the outputs viewed (the fusions stand) and with every
    non-constant tensor viewed"""
    for v in ("BAND_HIP_FUSION", "BAND_HIP_FUSED_ATTENTION", "BAND_HIP_FUSED_LAYERNORM_F32"):
        monkeypatch.delenv(v, raising=False)
    buf, xs, refs = model_refs[name]
    m, ex, key = _exec(buf, 71)
    om = OModel(buf)
    kernels = ex.LaunchKernels(key)
    if name in G.TEXT_ENCODERS:
        assert kernels.count(G.KERNEL) == 1 and kernels[0] == G.KERNEL, kernels
    else:
        assert G.KERNEL in kernels and "concat_kernel" in kernels and any(k.startswith("reindex_") for k in kernels)
    watch = [t.index for t in om.tensors if not t.is_const] if all_tensors else list(ex.GetOutputs(key))
    views = {t: ex.GetTensorView(key, t) for t in watch}
    t_in = ex.GetInputs(key)[0]
    for i in range(3):
        ex.GetTensorView(key, t_in).GetData()[...] = xs[i]
        assert ex.ExecuteSubgraph(key).ok()
        for t, v in views.items():
            _compare(name, t, v.GetData(), refs[i][t])


def test_runtime_index_out_of_range_on_the_executor(gpu_lib, monkeypatch):
    """indices axis_size and axis_size + 1 into an activation params of 6 rows of 16 bytes: a wrong guard would read
    bytes 96 .. 127 of the tensor's own 256-byte arena slot, nothing else.  A zero row, the pass succeeds, eager and
    replayed (negative indices: the launcher cases, which have guard rows in front)"""
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    x = G.fill((6, 16), np.int8)
    buf = G.raw_gather((6, 16), [0, 0, 0, 0], runtime_indices=True)
    m, ex, key = _exec(buf, 72)
    t_x, t_i = ex.GetInputs(key)
    t_out = ex.GetOutputs(key)[0]
    ex.GetTensorView(key, t_x).GetData()[...] = x
    for ids in ([5, 6, 0, 7], [6, 1, 7, 2], [3, 3, 6, 6]):
        ex.GetTensorView(key, t_i).GetData()[...] = np.asarray(ids, np.int32)
        assert ex.ExecuteSubgraph(key).ok()
        np.testing.assert_array_equal(ex.GetTensorView(key, t_out).GetData().reshape(4, 16), G.gather_ref(x, ids))


@pytest.mark.parametrize("name", ["text_encoder_i8", "text_encoder_hybrid", "pack_unpack_tile_i8"])
def test_job_batch_of_3_equals_the_single_runs(gpu_lib, monkeypatch, model_refs, name):
    """different ids per job; every slot equals that job's own single-job run byte for byte"""
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf, xs, refs = model_refs[name]
    m, ex, key = _exec(buf, 73)
    t_in = ex.GetInputs(key)[0]
    singles = []
    for x in xs:
        ex.GetTensorView(key, t_in).GetData()[...] = x
        assert ex.ExecuteSubgraph(key).ok()
        singles.append({t: ex.GetTensorView(key, t).GetData().copy() for t in ex.GetOutputs(key)})
    st = ex.PrepareJobBatches(m, key, 3)
    assert st.ok(), st.message()
    assert ex.MaxJobBatch(key) == 3
    for n in (2, 3):
        order = [(s + n) % 3 for s in range(n)]
        for s, i in enumerate(order):
            ex.GetJobSlotView(key, t_in, n, s).GetData()[...] = xs[i]
        for _ in range(2):  # eager, then the captured graph
            assert ex.ExecuteJobBatch(key, n).ok()
            for s, i in enumerate(order):
                for t in ex.GetOutputs(key):
                    got = ex.GetJobSlotView(key, t, n, s).GetData()
                    assert got.tobytes() == singles[i][t].tobytes(), "%s n=%d slot %d tensor %d" % (name, n, s, t)
                    _compare(name, t, got.reshape(refs[i][t].shape), refs[i][t])


def test_activation_gather_with_runtime_indices_runs_unbatched(gpu_lib, monkeypatch):
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf = G.raw_gather((1, 4, 4, 8), [1, 2], axis=1, runtime_indices=True)
    m, ex, key = _exec(buf, 74)
    st = ex.PrepareJobBatches(m, key, 3)
    assert not st.ok() and "job batching: GATHER with runtime indices into an activation params" in st.message()
    assert ex.MaxJobBatch(key) == 1
    x = G.fill((1, 4, 4, 8), np.int8)
    t_x, t_i = ex.GetInputs(key)
    ex.GetTensorView(key, t_x).GetData()[...] = x
    ex.GetTensorView(key, t_i).GetData()[...] = np.array([3, 0], np.int32)
    assert ex.ExecuteSubgraph(key).ok()
    np.testing.assert_array_equal(ex.GetTensorView(key, ex.GetOutputs(key)[0]).GetData().reshape(1, 2, 4, 8),
                                  x[:, [3, 0]])


def _engine_outputs(devices, path, xs, n_out):
    from band_amd.engine import Engine, JobStatus, Model, SchedulerType, make_config, kBandOk
    e = Engine(make_config([SchedulerType.kRoundRobin], devices, num_threads=[1] * len(devices)))
    m = Model()
    assert m.FromPath(path)
    assert e.RegisterModel(m)
    assert e.GetNumOutputTensors(m) == n_out
    res, workers = [], set()
    for x in xs:
        t = e.CreateInputTensor(m, 0)
        assert t.data().dtype == np.int32
        t.data()[...] = x
        outs = [e.CreateOutputTensor(m, k) for k in range(n_out)]
        h = e.RequestAsync(m, [t])
        assert h >= 0 and e.Wait(h, outs) == kBandOk
        r = e.GetJobRecord(h)
        assert r.status == JobStatus.kSuccess
        workers.add(r.worker_id)
        res.append([o.data().copy() for o in outs])
    e.close()
    return res, workers


def test_engine_cpu_and_gpu_workers_serve_the_text_encoder(gpu_lib, tmp_path, monkeypatch, model_refs):
    """round robin over a kCPU and a kGPU worker: both register the whole model (no unsupported op on either),
    both answer, and every output equals the CPU-only engine's and the reference"""
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf, xs, refs = model_refs["text_encoder_i8"]
    path = str(tmp_path / "text_encoder.tflite")
    with open(path, "wb") as f:
        f.write(buf)
    t_out = OModel(buf).outputs[0]
    feeds = [xs[i % 3] for i in range(4)]
    mixed, workers = _engine_outputs([DeviceFlag.kCPU, DeviceFlag.kGPU], path, feeds, 1)
    assert workers == {0, 1}
    cpu_only, _ = _engine_outputs([DeviceFlag.kCPU], path, feeds, 1)
    for i, (a, b) in enumerate(zip(mixed, cpu_only)):
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[0].reshape(refs[i % 3][t_out].shape), refs[i % 3][t_out])


# ---- the opt-in fusions still fire behind a GATHER ------------------------------------------
def test_fused_attention_behind_a_gather(gpu_lib, monkeypatch, model_refs):
    """BAND_HIP_FUSED_ATTENTION=1: one attention_i8_kernel per block, as for encoder_block, no bmm / softmax / head
    TRANSPOSE launch; the gather launch is a member of nothing; outputs exact"""
    from tests import attention_models as A
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf, xs, refs = model_refs["text_encoder_i8"]
    m0, ex0, key0 = _exec(buf, 75)
    plain = ex0.LaunchKernels(key0)
    monkeypatch.setenv("BAND_HIP_FUSED_ATTENTION", "1")
    m, ex, key = _exec(buf, 76)
    kernels = ex.LaunchKernels(key)
    enc = A.MODELS["encoder_17_48_3_96"]()
    me, exe, keye = _exec(enc, 77)
    per_block = exe.LaunchKernels(keye)
    assert kernels.count(A.KERNEL) == per_block.count(A.KERNEL) == 1, kernels
    assert not [k for k in kernels if k in ("bmm_mfma_kernel", "softmax_kernel")], kernels
    assert kernels.count(G.KERNEL) == 1 and kernels[0] == G.KERNEL
    # the block's launches are the encoder_block's own: text_encoder adds the gather, the position ADD, one
    # LayerNorm, the token-0 slice and the classifier around them
    assert len(kernels) == len(per_block) + 5, (kernels, per_block)
    assert len(plain) - len(kernels) == 6  # two products, the softmax and three head TRANSPOSEs leave; one launch comes
    t_in = ex.GetInputs(key)[0]
    for i in range(3):
        ex.GetTensorView(key, t_in).GetData()[...] = xs[i]
        assert ex.ExecuteSubgraph(key).ok()
        for t in ex.GetOutputs(key):
            np.testing.assert_array_equal(ex.GetTensorView(key, t).GetData().reshape(refs[i][t].shape), refs[i][t])


def test_fused_layernorm_f32_behind_a_gather(gpu_lib, monkeypatch, model_refs):
    """BAND_HIP_FUSED_LAYERNORM_F32=1 on the hybrid model: three layernorm_f32_kernel launches (the one up front and
    the block's two), no MEAN launch left, the block's launches as encoder_block's; the first LayerNorm - the one that
    reads what GATHER and the position ADD made - equals the rule of tests.layernorm_f32_models bit for bit"""
    from tests import hybrid_models as Y
    from tests import layernorm_f32_models as L
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    monkeypatch.setenv(L.FLAG, "1")
    buf, xs, refs = model_refs["text_encoder_hybrid"]
    om = OModel(buf)
    lns = L.layer_norms(om)
    assert len(lns) == 3
    m, ex, key = _exec(buf, 78)
    first = lns[0]
    vx, vy = ex.GetTensorView(key, first[0]), ex.GetTensorView(key, first[4])  # both are read by later ops anyway
    kernels = ex.LaunchKernels(key)
    enc = Y.MODELS["encoder_17_48_3_96_symmetric"]()
    me, exe, keye = _exec(enc, 79)
    per_block = exe.LaunchKernels(keye)
    assert per_block.count(L.KERNEL) == 2 and len(per_block) == 20, per_block
    assert kernels.count(L.KERNEL) == 3 and "mean_kernel" not in kernels, kernels
    assert kernels.count(Y.DQ_KERNEL) == per_block.count(Y.DQ_KERNEL) + 1  # the classifier's own row quantisation
    assert kernels.count(G.KERNEL) == 1 and kernels[0] == G.KERNEL
    assert len(kernels) == len(per_block) + 6, (kernels, per_block)  # gather, ADD, LayerNorm, slice, quantise + classifier
    t_in, t_out = ex.GetInputs(key)[0], ex.GetOutputs(key)[0]
    for i in range(3):
        ex.GetTensorView(key, t_in).GetData()[...] = xs[i]
        assert ex.ExecuteSubgraph(key).ok()
        y = L.model_layernorm(om, first, vx.GetData())
        np.testing.assert_array_equal(vy.GetData().reshape(y.shape).view(np.uint32), y.view(np.uint32))
        assert np.isfinite(ex.GetTensorView(key, t_out).GetData()).all()
