"""The masked form of the fused int8 attention launch on the MI355X:
bh_attention_i8 with a bias on every case of tests.mask_models.launcher_cases in
both requantisation forms (the kernel name, attention_bias_i8_kernel, is
asserted first; the 0xff bytes around the output must stay), the same cases
through the default sequence bh_batch_matmul_i8 -> bh_eltwise_i8 ->
bh_softmax_i8 -> bh_batch_matmul_i8, what the launcher refuses, and the models
with an ADD on their scores through the kGPU executor (tests.mask_models.MODELS).

Reference: tests.mask_models (the oracle's FULLY_CONNECTED per batch slice, the
oracle's add and softmax) and run_reference for models; everything is compared
with assert_array_equal."""
import ctypes

import numpy as np
import pytest

from tests import mask_models as M

pytestmark = pytest.mark.gpu

CASES = M.launcher_cases()


@pytest.fixture(scope="module")
def refs():
    out = {}
    for c in CASES:
        masked = c.masked()
        out[c.name] = (masked, c.ctx(masked))
    return out


@pytest.mark.parametrize("fast", [0, 1], ids=["two_step", "single_step"])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_masked_attention_launcher(gpu_lib, refs, case, fast):
    np.testing.assert_array_equal(M.launch(case, gpu_lib, requant_fast=fast), refs[case.name][1], err_msg=case.name)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_default_sequence_stores_the_same_bytes(gpu_lib, refs, case):
    """the four launches the fused one replaces, on the same operands: their masked scores and their context are the
    reference's, hence the fused launch's"""
    masked, ctx = M.launch_default_sequence(case, gpu_lib)
    np.testing.assert_array_equal(masked, refs[case.name][0], err_msg=case.name)
    np.testing.assert_array_equal(ctx, refs[case.name][1], err_msg=case.name)
    np.testing.assert_array_equal(M.launch(case, gpu_lib), ctx, err_msg=case.name)


def test_identity_bias_on_the_sum_order_rows(gpu_lib):
    """a bias at its zero point under ADD scales that reproduce the scores: the rows whose bytes change when the
    softmax's row sum is reversed or pairwise still come out as the in-order sum gives them"""
    case, rev_rows, pair_rows = M.identity_case()
    s = case.scores()
    np.testing.assert_array_equal(case.masked(s), s)
    assert len(rev_rows) > 0 and len(pair_rows) > 0
    np.testing.assert_array_equal(M.launch(case, gpu_lib), case.ctx(s))


@pytest.mark.parametrize("name,change,reason", M.refused_params(), ids=[r[0] for r in M.refused_params()])
def test_masked_attention_refuses_bad_parameters(gpu_lib, name, change, reason):
    p, bufs, read = M.prepare(M.valid_case(), device=True)
    assert gpu_lib.bh_attention_i8_kernel(ctypes.byref(p)) == M.KERNEL.encode()
    change(p)
    assert gpu_lib.bh_attention_i8_kernel(ctypes.byref(p)) == b""
    assert gpu_lib.bh_attention_i8(ctypes.byref(p), None) != 0
    msg = gpu_lib.bh_last_error().decode()
    assert msg.startswith("bh_attention_i8: ") and reason in msg, msg
    assert (bufs[3].download(np.uint8, (bufs[3].nbytes,)) == 0xff).all()


# ---- models --------------------------------------------------------------------------------
from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey  # noqa: E402
from oracle.tflite_fb import Model as OModel  # noqa: E402
from tests import attention_models as A  # noqa: E402
from tests.graph_reference import run_reference  # noqa: E402

FLAG = "BAND_HIP_FUSED_ATTENTION"
REPLACED = ("bmm_mfma_kernel", "softmax_kernel")


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
    for name, build in M.MODELS.items():
        buf = build()
        xs = [M.model_inputs(buf, seed=s) for s in range(5)]
        out[name] = (buf, xs, [run_reference(buf, x) for x in xs])
    return out


def _kernels(ex, key):
    return [r["kernel"] for r in ex.ProfileSubgraph(key, iters=1)]


def _set_inputs(ex, key, x):
    for t, v in x.items():
        ex.GetTensorView(key, t).GetData()[...] = v


def _check_outputs(ex, key, ref, msg):
    for t in ex.GetOutputs(key):
        np.testing.assert_array_equal(ex.GetTensorView(key, t).GetData().reshape(ref[t].shape), ref[t], err_msg=msg)


def _fused(monkeypatch, on=True):
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    if on:
        monkeypatch.setenv(FLAG, "1")
    else:
        monkeypatch.delenv(FLAG, raising=False)


@pytest.mark.parametrize("name", sorted(M.MODELS))
def test_masked_models_fused(gpu_lib, monkeypatch, model_refs, name):
    """an eager pass, then the captured graph twice: one attention_bias_i8_kernel, no bmm_mfma_kernel, softmax_kernel
    or head-TRANSPOSE reindex launch, and of the two eltwise launches (the ADD on the scores, the residual ADD) the
    residual one alone; then every tensor viewed: the subgraph re-lowers unfused and every tensor is right"""
    _fused(monkeypatch)
    buf, xs, refs_ = model_refs[name]
    m, ex, key = _exec(buf, 81)
    om = OModel(buf)
    kernels = _kernels(ex, key)
    assert kernels.count(M.KERNEL) == 1 and A.KERNEL not in kernels, kernels
    assert not [k for k in kernels if k in REPLACED or k.startswith("reindex")], kernels
    encoder = "encoder" in name
    assert kernels.count("eltwise_kernel") == (2 if encoder else 1), kernels  # the residual ADDs alone
    assert kernels.count("layernorm_i8_kernel") == (2 if encoder else 0), kernels
    for i in range(3):
        _set_inputs(ex, key, xs[i])
        assert ex.ExecuteSubgraph(key).ok()
        _check_outputs(ex, key, refs_[i], "%s pass %d" % (name, i))
    views = {t.index: ex.GetTensorView(key, t.index) for t in om.tensors if not t.is_const}
    kernels = _kernels(ex, key)
    assert M.KERNEL not in kernels and kernels.count("bmm_mfma_kernel") == 2 and kernels.count("softmax_kernel") == 1
    assert encoder or kernels.count("eltwise_kernel") == 2, kernels
    for i in range(3, 5):
        _set_inputs(ex, key, xs[i])
        assert ex.ExecuteSubgraph(key).ok()
        for t, v in views.items():
            np.testing.assert_array_equal(v.GetData().reshape(refs_[i][t].shape), refs_[i][t],
                                          err_msg="%s tensor %d" % (name, t))


@pytest.mark.parametrize("name", sorted(M.MODELS))
def test_flag_unset_leaves_the_four_launches(gpu_lib, monkeypatch, model_refs, name):
    _fused(monkeypatch, on=False)
    buf, xs, refs_ = model_refs[name]
    m, ex, key = _exec(buf, 82)
    kernels = _kernels(ex, key)
    assert M.KERNEL not in kernels and kernels.count("bmm_mfma_kernel") == 2 and kernels.count("softmax_kernel") == 1
    assert kernels.count("eltwise_kernel") == (3 if "encoder" in name else 2), kernels
    for i in range(2):  # eager, then the captured graph
        _set_inputs(ex, key, xs[i])
        assert ex.ExecuteSubgraph(key).ok()
        _check_outputs(ex, key, refs_[i], "unfused")


@pytest.mark.parametrize("kind", M.UNFUSABLE)
def test_a_refused_pattern_keeps_its_four_launches(gpu_lib, monkeypatch, kind):
    """with the flag set: a SUB in the ADD's place, an ADD of the scores to themselves, an ADD the launcher's check
    refuses (keys 1,025) each keep BATCH_MATMUL, the eltwise launch, SOFTMAX and BATCH_MATMUL,
    and the outputs are right, eager and replayed"""
    _fused(monkeypatch)
    buf = M.unfusable_model(kind)
    x = M.model_inputs(buf, seed=2)
    ref = run_reference(buf, x)
    m, ex, key = _exec(buf, 85)
    kernels = _kernels(ex, key)
    assert kernels == ["bmm_mfma_kernel", "eltwise_kernel", "softmax_kernel", "bmm_mfma_kernel"], kernels
    for _ in range(2):
        _set_inputs(ex, key, x)
        assert ex.ExecuteSubgraph(key).ok()
        _check_outputs(ex, key, ref, kind)


@pytest.mark.parametrize("which", ["scores", "masked"])
def test_a_view_of_the_scores_keeps_the_four_launches(gpu_lib, monkeypatch, model_refs, which):
    """the scores, or the ADD's output, viewed: neither is private to the pattern any more"""
    _fused(monkeypatch)
    buf, xs, refs_ = model_refs["relative_17_48_3"]
    m, ex, key = _exec(buf, 83)
    (sc, ms, pr, ctx, bias), = M.masked_attention_tensors(buf)
    t = sc if which == "scores" else ms
    view = ex.GetTensorView(key, t)
    kernels = _kernels(ex, key)
    assert M.KERNEL not in kernels and kernels.count("bmm_mfma_kernel") == 2 and kernels.count("softmax_kernel") == 1
    for i in range(2):
        _set_inputs(ex, key, xs[i])
        assert ex.ExecuteSubgraph(key).ok()
        np.testing.assert_array_equal(view.GetData().reshape(refs_[i][t].shape), refs_[i][t])
        _check_outputs(ex, key, refs_[i], which)


@pytest.mark.parametrize("name", ["causal_17_48_3", "padded_one_17_48_3"])
def test_masked_models_job_batches(gpu_lib, monkeypatch, model_refs, name):
    """job batches 2, 3 and 5 against single runs; the padding mask's axis 0 is the job axis, and every variant is
    still one fused launch"""
    _fused(monkeypatch)
    buf, xs, refs_ = model_refs[name]
    m, ex, key = _exec(buf, 84)
    st = ex.PrepareJobBatches(m, key, 5)
    assert st.ok(), st.message()
    assert ex.MaxJobBatch(key) == 5
    for n in (2, 3, 5):
        assert ex.JobBatchLaunchKernels(key, n).count(M.KERNEL) == 1
        order = [(s + n) % 5 for s in range(n)]
        for s, i in enumerate(order):
            for t, v in xs[i].items():
                ex.GetJobSlotView(key, t, n, s).GetData()[...] = v
        for _ in range(2):
            assert ex.ExecuteJobBatch(key, n).ok()
            for s, i in enumerate(order):
                for t in ex.GetOutputs(key):
                    got = ex.GetJobSlotView(key, t, n, s).GetData()
                    np.testing.assert_array_equal(got.reshape(refs_[i][t].shape), refs_[i][t],
                                                  err_msg="%s n=%d slot %d" % (name, n, s))


def test_engine_gpu_worker_serves_the_padded_block(gpu_lib, tmp_path, monkeypatch, model_refs):
    from band_amd.engine import Engine, JobStatus, Model, SchedulerType, make_config, kBandOk
    _fused(monkeypatch)
    buf, xs, refs_ = model_refs["padded_17_48_3"]
    om = OModel(buf)
    e = Engine(make_config([SchedulerType.kRoundRobin], [DeviceFlag.kGPU]))
    path = str(tmp_path / "padded_block.tflite")
    with open(path, "wb") as f:
        f.write(buf)
    m = Model()
    assert m.FromPath(path)
    assert e.RegisterModel(m)
    ins = []
    for k, t in enumerate(om.inputs):
        ten = e.CreateInputTensor(m, k)
        ten.data()[...] = xs[0][t]
        ins.append(ten)
    outs = [e.CreateOutputTensor(m, 0)]
    h = e.RequestAsync(m, ins)
    assert h >= 0 and e.Wait(h, outs) == kBandOk
    assert e.GetJobRecord(h).status == JobStatus.kSuccess
    np.testing.assert_array_equal(outs[0].data().reshape(refs_[0][om.outputs[0]].shape), refs_[0][om.outputs[0]])
    e.close()


def test_float_causal_rows_ignore_later_tokens_on_the_gpu(gpu_lib):
    from tests.test_attention_mask_cpu import float_causal_rows_ignore_later_tokens
    float_causal_rows_ignore_later_tokens(DeviceFlag.kGPU, 1)
