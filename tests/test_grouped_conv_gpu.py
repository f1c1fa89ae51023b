"""Grouped CONV_2D on the MI355X: bh_conv2d_grouped_i8 on every case (dtype x
requantisation mode x form, residual ADD, byte table, bytes past the output),
its refusals, and ShuffleNet-v1 / conv -> ADD / conv -> RELU6 models on the
kGPU executor (eager, captured graph, job batches) and through the engine.
Expected bytes: the oracle's dense conv per group (tests/grouped_models.py)."""
import ctypes

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey
from oracle.tflite_fb import Model as OModel
from tests import grouped_models as G
from tests import reindex_models as R
from tests.graph_reference import run_reference

pytestmark = pytest.mark.gpu

RANDOM = G.random_cases()
DIRECTED = G.directed_cases()
KERNEL = "conv_grouped_mfma_kernel"


@pytest.fixture(scope="module")
def refs():
    out = {}
    for cid, i, dt, act in RANDOM:
        case = G.make_case(i, dt, act)
        ref = G.grouped_ref(case)
        G.check_reference(case, ref)
        out[cid] = (case, ref)
    return out


# ---- the launcher ------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c[0] for c in RANDOM])
def test_launcher_random(gpu_lib, refs, cid):
    """every requantisation mode x form (automatic routing and each pinned form)"""
    case, ref = refs[cid]
    for fast in (None, False):
        for hint in (0,) + G.forms_for(case.shape):
            case.cc.requant_fast, case.cc.kernel_hint = fast, hint
            np.testing.assert_array_equal(G.launch(case, gpu_lib, True), ref, err_msg="fast %s hint %d" % (fast, hint))
    case.cc.requant_fast, case.cc.kernel_hint = None, 0


@pytest.mark.parametrize("cid,case", DIRECTED, ids=[c[0] for c in DIRECTED])
def test_launcher_directed(gpu_lib, cid, case):
    ref = G.grouped_ref(case)
    G.check_directed(cid, case, ref)
    for fast in (None, False):
        for hint in G.forms_for(case.shape):
            case.cc.requant_fast, case.cc.kernel_hint = fast, hint
            np.testing.assert_array_equal(G.launch(case, gpu_lib, True), ref, err_msg="fast %s hint %d" % (fast, hint))


@pytest.mark.parametrize("cid", [c[0] for c in RANDOM if c[3] == G.NONE])
def test_launcher_residual_and_table(gpu_lib, refs, cid):
    case, ref = refs[cid]
    r, set_add, z, table = G.residual_of(case, ref, 900)
    for fast in (None, False):
        case.cc.requant_fast = fast
        np.testing.assert_array_equal(G.launch(case, gpu_lib, True, residual=(r, set_add)), z)
        np.testing.assert_array_equal(G.launch(case, gpu_lib, True, table=table).view(np.uint8),
                                      table[ref.view(np.uint8)])
        both = table[z.view(np.uint8)]
        np.testing.assert_array_equal(G.launch(case, gpu_lib, True, residual=(r, set_add), table=table).view(np.uint8),
                                      both)
    case.cc.requant_fast = None


def test_launcher_refuses_bad_parameters(gpu_lib):
    case = G.make_case(0, np.int8, G.NONE)
    keep = []
    p = G.grouped_params(case, gpu_lib, keep, True)
    assert gpu_lib.bh_conv2d_grouped_i8_kernel(ctypes.byref(p)) == KERNEL.encode()

    def refused(q):
        assert gpu_lib.bh_conv2d_grouped_i8(ctypes.byref(q), None) != 0
        assert b"bh_conv2d_grouped_i8" in gpu_lib.bh_last_error()
        assert gpu_lib.bh_conv2d_grouped_i8_kernel(ctypes.byref(q)) == b""
    for groups in (0, 3, 4, 5):  # ic = 6, oc = 10: 3 divides only ic, 5 only oc
        refused(G.grouped_params(case, gpu_lib, keep, True, groups=groups))
    for name in ("input", "output", "weights", "bias_eff", "mult", "shift"):
        q = G.grouped_params(case, gpu_lib, keep, True)
        setattr(q.conv, name, None)
        refused(q)
    q = G.grouped_params(case, gpu_lib, keep, True)
    q.conv.k_pad = 0
    refused(q)
    assert gpu_lib.bh_conv2d_grouped_i8(None, None) != 0


# ---- models ----------------------------------------------------------------------------------
def _exec(buf, mid):
    m = HipModel(mid)
    assert m.FromBuffer(buf).ok()
    ex = HipModelExecutor(mid, 1, DeviceFlag.kGPU)
    assert ex.InvestigateModelSpec(m).unsupported_ops[DeviceFlag.kGPU] == set()
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    ex._model_ref = m
    return m, ex, SubgraphKey(mid, 1)


def _same(name, t, got, ref):
    assert got.dtype == ref.dtype, (name, t)
    np.testing.assert_array_equal(got.reshape(ref.shape), ref, err_msg="%s tensor %d" % (name, t))


@pytest.fixture(scope="module")
def shuffle_refs():
    """per dtype: the model, 3 inputs and run_reference of each"""
    out = {}
    for dt in G.DTYPES:
        buf = G.shufflenet_small(dt)
        xs = [R.zoo_input(buf, seed=20 + i) for i in range(3)]
        out[np.dtype(dt).name] = (buf, xs, [run_reference(buf, x) for x in xs])
    return out


@pytest.mark.parametrize("name", ["out_channels", "in_channels", "float32"])
def test_gpu_spec_refusals(gpu_lib, name):
    from tests.test_grouped_conv_cpu import _refusals
    build, reason = _refusals()[name]
    m = HipModel(70)
    assert m.FromBuffer(build()).ok()
    ex = HipModelExecutor(70, 1, DeviceFlag.kGPU)
    assert ex.InvestigateModelSpec(m).unsupported_ops[DeviceFlag.kGPU] == {0}
    st = ex.PrepareSubgraph(m)
    assert not st.ok() and reason in st.message(), st.message()


@pytest.mark.parametrize("all_tensors", [False, True], ids=["outputs", "every_tensor"])
@pytest.mark.parametrize("dtype", ["int8", "uint8"])
def test_shufflenet_gpu_executor(gpu_lib, monkeypatch, shuffle_refs, dtype, all_tensors):
    """an eager pass, then the captured graph twice; the whole model is one
    subgraph, every grouped layer one conv_grouped_mfma_kernel launch"""
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf, xs, refs = shuffle_refs[dtype]
    m, ex, key = _exec(buf, 71)
    om = OModel(buf)
    n_grouped = sum(G.is_grouped(om, o) for o in om.operators)
    assert n_grouped >= 5
    rows = ex.ProfileSubgraph(key, iters=1)
    grouped_ops = {i for i, o in enumerate(om.operators) if G.is_grouped(om, o)}
    by_op = {}
    for r in rows:
        by_op.setdefault(r["op_index"], []).append(r["kernel"])
    for i in grouped_ops:  # one launch each, the grouped kernel: no reindex / concat launches standing in
        assert len(by_op[i]) == 1 and by_op[i][0].startswith(KERNEL), (i, by_op[i])
    assert sum(k.startswith(KERNEL) for r in rows for k in [r["kernel"]]) == n_grouped
    watch = list(ex.GetOutputs(key))
    if all_tensors:
        watch = [t.index for t in om.tensors if not t.is_const]
    views = {t: ex.GetTensorView(key, t) for t in watch}
    t_in = ex.GetInputs(key)[0]
    for i in range(3):
        ex.GetTensorView(key, t_in).GetData()[...] = xs[i]
        assert ex.ExecuteSubgraph(key).ok()
        for t, v in views.items():
            _same("shufflenet_v1 %s" % dtype, t, v.GetData(), refs[i][t])


def test_shufflenet_job_batches(gpu_lib, monkeypatch, shuffle_refs):
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf, xs, refs = shuffle_refs["int8"]
    m, ex, key = _exec(buf, 72)
    st = ex.PrepareJobBatches(m, key, 3)
    assert st.ok(), st.message()
    assert ex.MaxJobBatch(key) == 3
    t_in = ex.GetInputs(key)[0]
    for n in (2, 3):
        order = [(s + n) % 3 for s in range(n)]
        for s, i in enumerate(order):
            ex.GetJobSlotView(key, t_in, n, s).GetData()[...] = xs[i]
        for _ in range(2):
            assert ex.ExecuteJobBatch(key, n).ok()
            for s, i in enumerate(order):
                for t in ex.GetOutputs(key):
                    got = ex.GetJobSlotView(key, t, n, s).GetData()
                    _same("n=%d slot %d" % (n, s), t, got.reshape(refs[i][t].shape), refs[i][t])


@pytest.mark.parametrize("build", [G.conv_then_add, G.conv_then_relu6], ids=["add", "relu6"])
@pytest.mark.parametrize("dtype", G.DTYPES, ids=["int8", "uint8"])
def test_following_add_and_relu6(gpu_lib, monkeypatch, build, dtype):
    """with only the output viewed the ADD / RELU6 folds into the grouped
    launch's epilogue; with every tensor viewed it stands alone"""
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf = build(dtype)
    om = OModel(buf)
    xs = [R.zoo_input(buf, seed=30 + i) for i in range(3)]
    refs = [run_reference(buf, x) for x in xs]
    for all_tensors in (False, True):
        m, ex, key = _exec(buf, 73)
        watch = [t.index for t in om.tensors if not t.is_const] if all_tensors else list(ex.GetOutputs(key))
        views = {t: ex.GetTensorView(key, t) for t in watch}
        kernels = [r["kernel"] for r in ex.ProfileSubgraph(key, iters=1)]
        assert kernels[0].startswith(KERNEL), kernels
        assert len(kernels) == (2 if all_tensors else 1), kernels
        for i in range(3):
            ex.GetTensorView(key, ex.GetInputs(key)[0]).GetData()[...] = xs[i]
            assert ex.ExecuteSubgraph(key).ok()
            for t, v in views.items():
                _same(build.__name__, t, v.GetData(), refs[i][t])


def test_engine_one_gpu_worker_whole_model(gpu_lib, tmp_path, monkeypatch):
    """an engine whose only worker is a GPU worker registers ShuffleNet-v1 - every
    op has to be in the kGPU set - as one whole-model subgraph and answers a request"""
    from band_amd.engine import Engine, JobStatus, Model, SchedulerType, make_config, kBandOk
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf = G.shufflenet_small(np.int8)
    om = OModel(buf)
    path = str(tmp_path / "shufflenet_v1.tflite")
    with open(path, "wb") as f:
        f.write(buf)
    e = Engine(make_config([SchedulerType.kRoundRobin], [DeviceFlag.kGPU]))
    m = Model()
    assert m.FromPath(path)
    assert e.RegisterModel(m)
    subs = e.GetSubgraphs(m)
    assert len(subs) == 1 and subs[0][0] == 0, subs  # one subgraph: the whole model on the GPU worker
    x = R.zoo_input(buf, seed=50)
    ref = run_reference(buf, x)[om.outputs[0]]
    t = e.CreateInputTensor(m, 0)
    t.data()[...] = x
    out = [e.CreateOutputTensor(m, 0)]
    h = e.RequestAsync(m, [t])
    assert h >= 0 and e.Wait(h, out) == kBandOk
    assert e.GetJobRecord(h).status == JobStatus.kSuccess
    np.testing.assert_array_equal(out[0].data().reshape(ref.shape), ref)
    e.close()


def test_engine_gpu_and_cpu_worker(gpu_lib, tmp_path, monkeypatch):
    """one engine with a GPU and a CPU worker registers ShuffleNet-v1 (every op
    is in both workers' sets); requests pinned to each worker are answered by
    that worker, bit-exact"""
    from band_amd.engine import (Engine, JobStatus, Model, RequestOptionGetDefault, SchedulerType, make_config,
                                 kBandOk)
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf = G.shufflenet_small(np.int8)
    om = OModel(buf)
    path = str(tmp_path / "shufflenet_v1.tflite")
    with open(path, "wb") as f:
        f.write(buf)
    e = Engine(make_config([SchedulerType.kFixedWorker], [DeviceFlag.kGPU, DeviceFlag.kCPU], num_threads=[1, 2]))
    m = Model()
    assert m.FromPath(path)
    assert e.RegisterModel(m)
    assert e.GetWorkerDevice(0) == DeviceFlag.kGPU and e.GetWorkerDevice(1) == DeviceFlag.kCPU
    assert {k[0] for k in e.GetSubgraphs(m)} == {0, 1}  # both workers prepared the model
    served = []
    for i, worker in enumerate((0, 1, 1, 0)):
        x = R.zoo_input(buf, seed=40 + i)
        ref = run_reference(buf, x)[om.outputs[0]]
        t, out = e.CreateInputTensor(m, 0), [e.CreateOutputTensor(m, 0)]
        t.data()[...] = x
        opt = RequestOptionGetDefault()
        opt.target_worker = worker
        h = e.RequestAsync(m, [t], option=opt)
        assert h >= 0 and e.Wait(h, out) == kBandOk
        rec = e.GetJobRecord(h)
        assert rec.status == JobStatus.kSuccess
        served.append(rec.worker_id)
        np.testing.assert_array_equal(out[0].data().reshape(ref.shape), ref, err_msg="worker %d" % worker)
    assert served == [0, 1, 1, 0]
    e.close()


def test_concurrent_execute_subgraph_coalesces(gpu_lib, monkeypatch):
    """4 executors of ShuffleNet-v1 on one GPU call ExecuteSubgraph at the same
    moment, round after round, each with its own input (the pattern of
    tests/test_coalescer_gpu.py): the coalescer runs them as job-batch passes
    with no grouped-conv rule of its own, and every caller gets its own bytes"""
    import threading
    from band_amd import SetWorkerDevice
    from band_amd.backend import CoalescerStats
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    monkeypatch.setenv("BAND_HIP_COALESCE", "4")
    monkeypatch.setenv("BAND_HIP_COALESCE_LANES", "2")
    buf = G.shufflenet_small(np.int8)
    om = OModel(buf)
    xs = [R.zoo_input(buf, seed=60 + i) for i in range(4)]
    refs = [run_reference(buf, x) for x in xs]
    mid = 74
    m = HipModel(mid)
    assert m.FromBuffer(buf).ok()
    W = 4
    execs = []
    for w in range(W):
        SetWorkerDevice(200 + w, 0)
        ex = HipModelExecutor(mid, 200 + w, DeviceFlag.kGPU)
        assert ex.PrepareSubgraph(m).ok()
        execs.append((ex, SubgraphKey(mid, 200 + w)))
    for ex, _ in execs:
        assert ex.Coalescer() == (W, True)
    CoalescerStats(reset=True)
    rounds = 6
    barrier = threading.Barrier(W)
    errors = []

    def run(tid):
        ex, key = execs[tid]
        try:
            for r in range(rounds):
                k = (tid + r) % len(xs)
                ex.GetTensorView(key, om.inputs[0]).GetData()[...] = xs[k]
                barrier.wait(timeout=60)
                st = ex.ExecuteSubgraph(key)
                assert st.ok(), st
                for o in om.outputs:
                    got = ex.GetTensorView(key, o).GetData()
                    np.testing.assert_array_equal(got, refs[k][o].reshape(got.shape),
                                                  err_msg="thread %d round %d output %d" % (tid, r, o))
        except BaseException as e:  # noqa: BLE001 - reported below
            errors.append(e)
            barrier.abort()

    ths = [threading.Thread(target=run, args=(t,)) for t in range(W)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in ths), "a coalesced call never returned"
    if errors:
        raise errors[0]
    s = CoalescerStats()
    assert s["calls"] == W * rounds, s
    assert s["group_passes"] > 0 and s["group_jobs"] >= 2 * s["group_passes"], s
